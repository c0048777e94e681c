/* ssw_host_align.inc -- host: ssw_align_batch, ssw_alignment_propagate.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* alignment                                                                            */
/* ---------------------------------------------------------------------------------- */
static int
align_batch_impl(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                 const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                 const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                 ssw_align_entry_t *state_io, int32_t *status, void *stream, int level,
                 const int32_t *only, int32_t n_only, const ssw_compact_plan_s *cp, bool bt,
                 bool *used_bt);

/* cp != NULL: d_senscr holds the plan's compact rows (ssw_host_compact.inc) */
static int
align_batch_levels(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                   const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                   const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                   ssw_align_entry_t *state_io, int32_t *status, void *stream,
                   const ssw_compact_plan_s *cp);

/* State alignment over HMMs of 1, 2, 4 or 5 emitting states (the transition matrices' shape
 * decides; senid is [total_phones][n_emit], state_io [total_phones * n_emit]):
 * viterbi_align_any_kernel (ssw_k2_anytopo.inc), one wave per utterance, state in an HBM
 * workspace, full tokens.  No shipped model takes this path; it is there so that a model the
 * reference accepts (hmm_vit_eval, src/hmm.c:741-759) is not refused. */
static int
align_batch_any(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts, const int32_t *frame_off,
                const int32_t *phone_off, const uint16_t *senid, const int16_t *tmatid,
                const int32_t *sf, const int32_t *ef, ssw_align_entry_t *state_io,
                int32_t *status, void *stream)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    const int ne = h->tp_n_state;
    if (n_utts <= 0)
        return 0;
    if (m->device == SSW_DEVICE_NONE) {
        ssw_set_error("model was loaded with device = SSW_DEVICE_NONE (tables only): no GPU, "
                      "no alignment -- there is no CPU fallback");
        return -1;
    }
    if (ne < 1 || ne > 5) { /* HMM_MAX_NSTATE, include/soundswallower/hmm.h */
        ssw_set_error("transition matrices of %d emitting states (the reference's limit is 5)", ne);
        return -1;
    }
    if (d_senscr == NULL || frame_off == NULL || phone_off == NULL || senid == NULL
        || tmatid == NULL || sf == NULL || ef == NULL || state_io == NULL || status == NULL) {
        ssw_set_error("ssw_align_batch: NULL argument");
        return -1;
    }
    if (frame_off[0] != 0 || phone_off[0] != 0) {
        ssw_set_error("ssw_align_batch: offsets must start at 0");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    const int total_phones = phone_off[n_utts];
    std::vector<AlignUtt> utts((size_t)n_utts);
    long long tok_total = 0;
    int max_phones = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (frame_off[u + 1] < frame_off[u] || phone_off[u + 1] < phone_off[u]) {
            ssw_set_error("ssw_align_batch: offsets must not decrease (utterance %d)", u);
            return -1;
        }
        AlignUtt &U = utts[(size_t)u];
        U.frame_off = frame_off[u];
        U.n_frames = frame_off[u + 1] - frame_off[u];
        U.phone_off = phone_off[u];
        U.n_phones = phone_off[u + 1] - phone_off[u];
        U.tok_off = tok_total;
        U.scr_off = (long long)U.frame_off * h->n_sen;
        U.scr_stride = h->n_sen;
        U.pad_ = 0;
        if (U.n_phones < 1) {
            ssw_set_error("utterance %d: %d phones, %d frames", u, U.n_phones, U.n_frames);
            return -1;
        }
        max_phones = std::max(max_phones, U.n_phones);
        tok_total += (long long)U.n_frames * U.n_phones * ne;
    }
    for (size_t i = 0; i < (size_t)total_phones * ne; ++i)
        if (senid[i] >= h->n_sen) {
            ssw_set_error("phone %zu: senone %d of %d", i / ne, senid[i], h->n_sen);
            return -1;
        }
    for (int p = 0; p < total_phones; ++p)
        if (tmatid[p] < 0 || tmatid[p] >= h->tp_n_tmat) {
            ssw_set_error("phone %d: transition matrix %d out of range", p, tmatid[p]);
            return -1;
        }
    for (int u = 0; u < n_utts; ++u)
        utts[(size_t)u].ws_off = (long long)u * G_COUNT * (max_phones + 1);
    WsLayout L;
    const size_t b_state = sizeof(ssw_align_entry_t) * (size_t)ne * total_phones;
    const size_t o_utts = L.in(utts.data(), sizeof(AlignUtt) * n_utts);
    const size_t o_senid = L.in(senid, sizeof(uint16_t) * (size_t)ne * total_phones,
                                sizeof(uint16_t) * (size_t)ne * total_phones + 16);
    const size_t o_tmatid = L.in(tmatid, sizeof(int16_t) * (size_t)total_phones,
                                 sizeof(int16_t) * (size_t)total_phones + 16);
    const size_t o_sf = L.in(sf, sizeof(int32_t) * (size_t)total_phones);
    const size_t o_ef = L.in(ef, sizeof(int32_t) * (size_t)total_phones);
    const size_t o_state = L.in(state_io, b_state);
    const size_t o_status = L.out(sizeof(int32_t) * n_utts);
    const size_t o_tok = L.out(sizeof(int2) * (size_t)(tok_total > 0 ? tok_total : 1));
    const size_t o_big = L.out(sizeof(int) * (size_t)n_utts * G_COUNT * (max_phones + 1));
    if (devbuf_reserve(m->align_ws, L.size(), "ssw_align_batch") < 0)
        return -1;
    unsigned char *ws = m->align_ws.p;
    /* utts | senid | tmatid | sf | ef | state in one copy */
    if (stage_upload(m, ws + o_utts, L.in_bytes(), st, [&](unsigned char *hs) { L.fill(hs, 0); }) < 0)
        return -1;
    AlignParams A;
    memset(&A, 0, sizeof(A));
    A.senscr = d_senscr;
    A.utts = reinterpret_cast<AlignUtt *>(ws + o_utts);
    A.senid = reinterpret_cast<uint16_t *>(ws + o_senid);
    A.tmatid = reinterpret_cast<int16_t *>(ws + o_tmatid);
    A.sf = reinterpret_cast<int32_t *>(ws + o_sf);
    A.ef = reinterpret_cast<int32_t *>(ws + o_ef);
    A.tp = m->d_tp;
    A.tokens = reinterpret_cast<int2 *>(ws + o_tok);
    A.state_io = reinterpret_cast<ssw_align_entry_t *>(ws + o_state);
    A.status = reinterpret_cast<int32_t *>(ws + o_status);
    A.n_sen = h->n_sen;
    A.n_utts = n_utts;
    A.max_phones = max_phones;
    A.big_ws = reinterpret_cast<int *>(ws + o_big);
    hipLaunchKernelGGL(viterbi_align_any_kernel, dim3(n_utts), dim3(64), 0, st, A, ne);
    HIP_OK(hipGetLastError());
    {
        const size_t b_status = align256(sizeof(int32_t) * (size_t)n_utts);
        int slot = 0;
        unsigned char *hs = stage_acquire(m, b_status + b_state, &slot);
        if (hs == NULL)
            return -1;
        HIP_OK(hipMemcpyAsync(hs, ws + o_status, sizeof(int32_t) * (size_t)n_utts,
                              hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hs + b_status, ws + o_state, b_state, hipMemcpyDeviceToHost, st));
        if (stage_release(m, slot, st) < 0)
            return -1;
        HIP_OK(hipStreamSynchronize(st));
        memcpy(status, hs, sizeof(int32_t) * (size_t)n_utts);
        memcpy(state_io, hs + b_status, b_state);
    }
    return 0;
}

extern "C" int
ssw_align_batch(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                ssw_align_entry_t *state_io, int32_t *status, void *stream)
{
    return align_batch_levels(m, d_senscr, n_utts, frame_off, phone_off, senid, tmatid, sf, ef,
                              state_io, status, stream, NULL);
}

static int
align_batch_levels(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                   const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                   const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                   ssw_align_entry_t *state_io, int32_t *status, void *stream,
                   const ssw_compact_plan_s *cp)
{
    /* Utterances beyond 1024 phones, three levels.  2: the sliding-window register kernel
     * (viterbi_align_win_kernel) with a banded token table; an utterance whose active range or
     * token bands outgrow it says so (-(1 << 30)) and the batch is run again at level 1: state in
     * LDS, or in HBM with the banded table; and from there at level 0 with the full
     * [frame][state] table, as rounds 1-2 allocated it.  SSW_ALIGN_BAND=0: level 0 at once;
     * SSW_ALIGN_WIN=0: never level 2. */
    refresh_knobs(m);
    if (m->h->tp != NULL && m->h->tp_n_state != 3) { /* hmm_vit_eval's other branches */
        if (cp != NULL) {
            ssw_set_error("compact score rows are built for 3-state HMMs");
            return -1;
        }
        return align_batch_any(m, d_senscr, n_utts, frame_off, phone_off, senid, tmatid, sf, ef,
                               state_io, status, stream);
    }
    int level = !m->kn.align_band ? 0 : !m->kn.align_win ? 1 : 2;
    /* Round 5, above the levels: utterances of up to 1024 phones go through the byte-token kernel
     * first (viterbi_align_mwb_kernel: 2-bit back-pointers, scores replayed along the path); the
     * ones it cannot follow (-(1 << 30): it has written nothing for them) are run again, they
     * alone, with the reference's full tokens.  SSW_ALIGN_BT=0: full tokens at once. */
    bool bt = m->kn.align_bt;
    /* Only the utterances that reported -(1 << 30) are run again one level down, and they start
     * from the state entries the caller passed in (state_io is in / out: a copy is kept while a
     * fall-back is possible, i.e. for batches with an utterance beyond 1024 phones or a forced
     * kernel) -- round 3 ran the whole batch again on whatever the failed level had copied back,
     * which was right only because an overflowed utterance skips its backtrace (ADVICE r3). */
    std::vector<ssw_align_entry_t> pristine;
    if (level > 0 && n_utts > 0 && phone_off != NULL && state_io != NULL && phone_off[n_utts] > 0) {
        int max_phones = 0;
        for (int u = 0; u < n_utts; ++u)
            max_phones = std::max(max_phones, phone_off[u + 1] - phone_off[u]);
        if (max_phones > 64 * SSW_ALIGN_MAX_WAVES || m->kn.align_kernel[0] != 0) {
            /* SSW_ALIGN_STATE_OUT_ONLY: what the caller's array holds on entry is not looked at --
             * the state a rerun starts from is the zeros the first run started from */
            if (m->align_state_out_only) {
                ssw_align_entry_t zero;
                memset(&zero, 0, sizeof(zero));
                pristine.assign(3 * (size_t)phone_off[n_utts], zero);
            } else
                pristine.assign(state_io, state_io + 3 * (size_t)phone_off[n_utts]);
        }
    }
    std::vector<int32_t> only; /* empty = every utterance */
    for (;;) {
        bool used_bt = false;
        int rc = align_batch_impl(m, d_senscr, n_utts, frame_off, phone_off, senid, tmatid, sf, ef,
                                  state_io, status, stream, level,
                                  only.empty() ? NULL : only.data(), (int32_t)only.size(), cp, bt,
                                  &used_bt);
        if (rc != 0 || (level == 0 && !used_bt))
            return rc;
        std::vector<int32_t> failed;
        if (only.empty()) {
            for (int u = 0; u < n_utts; ++u)
                if (status[u] == -(1 << 30))
                    failed.push_back(u);
        } else {
            for (int32_t u : only)
                if (status[u] == -(1 << 30))
                    failed.push_back(u);
        }
        if (failed.empty())
            return rc;
        if (used_bt) { /* the same level again without byte tokens; state_io of these is untouched */
            m->align_stats[1] += (int64_t)failed.size();
            bt = false;
            only.swap(failed);
            continue;
        }
        if (pristine.empty()) {
            /* a kernel reported an overflow in a batch for which no fall-back was foreseen (only
             * the sliding-window and banded kernels -- utterances beyond 1024 phones, or a
             * forced kernel -- can): without the caller's state entries the rerun would start
             * from whatever the failed level copied back (ADVICE r4): refuse instead */
            ssw_set_error("ssw_align_batch: internal error: utterance %d overflowed a kernel "
                          "that has no fall-back state kept", failed[0]);
            return -1;
        }
        if (!pristine.empty())
            for (int32_t u : failed)
                memcpy(state_io + 3 * (size_t)phone_off[u], pristine.data() + 3 * (size_t)phone_off[u],
                       sizeof(ssw_align_entry_t) * 3 * (size_t)(phone_off[u + 1] - phone_off[u]));
        only.swap(failed);
        --level;
    }
}

static int
align_batch_impl(ssw_model_t *m, const int16_t *d_senscr, int32_t n_utts,
                 const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                 const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                 ssw_align_entry_t *state_io, int32_t *status, void *stream, int level,
                 const int32_t *only, int32_t n_only, const ssw_compact_plan_s *cp, bool bt,
                 bool *used_bt)
{
    const bool allow_band = level >= 1;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    if (n_utts <= 0)
        return 0;
    if (m->device == SSW_DEVICE_NONE) {
        ssw_set_error("model was loaded with device = SSW_DEVICE_NONE (tables only): no GPU, "
                      "no alignment -- there is no CPU fallback");
        return -1;
    }
    if (h->tp == NULL || h->tp_n_state != 3) {
        ssw_set_error("alignment kernel needs 3-state transition matrices");
        return -1;
    }
    if (d_senscr == NULL || frame_off == NULL || phone_off == NULL || senid == NULL
        || tmatid == NULL || sf == NULL || ef == NULL || state_io == NULL || status == NULL) {
        ssw_set_error("ssw_align_batch: NULL argument");
        return -1;
    }
    if (frame_off[0] != 0 || phone_off[0] != 0) {
        ssw_set_error("ssw_align_batch: offsets must start at 0");
        return -1;
    }
    for (int u = 0; u < n_utts; ++u)
        if (frame_off[u + 1] < frame_off[u] || phone_off[u + 1] < phone_off[u]) {
            ssw_set_error("ssw_align_batch: offsets must not decrease (utterance %d)", u);
            return -1;
        }
    HIP_OK(hipSetDevice(m->device));
    const int total_phones = phone_off[n_utts];
    for (size_t i = 0; cp == NULL && i < (size_t)total_phones * 3; ++i)
        if (senid[i] >= h->n_sen) { /* would index past a score row on the device */
            ssw_set_error("phone %zu: senone %d of %d", i / 3, senid[i], h->n_sen);
            return -1;
        }
    /* the utterances this call runs: all of them, or the `only` list (a fall-back) */
    const int n_run = only != NULL ? n_only : n_utts;
    auto utt_of = [&](int i) { return only != NULL ? only[i] : i; };
    std::vector<AlignUtt> utts((size_t)n_run);
    long long tok_total = 0;
    int max_phones = 0;
    for (int i = 0; i < n_run; ++i)
        max_phones = std::max(max_phones, phone_off[utt_of(i) + 1] - phone_off[utt_of(i)]);
    /* SSW_ALIGN_KERNEL = "lds", "reg", "mw", "hbm", "win": tests and tuning */
    const char *mode = m->kn.align_kernel[0] != 0 ? m->kn.align_kernel : NULL;
    /* beyond 1024 phones: the sliding-window register kernel (level 2); else the state lives in
     * LDS, beyond what LDS holds (2,560 phones, about 550 words) in an HBM workspace
     * (viterbi_align_kernel<0, true>) */
    const size_t lds = (size_t)A_COUNT * (max_phones + 1) * sizeof(int);
    const bool win = level == 2
        && ((max_phones > 64 * SSW_ALIGN_MAX_WAVES && mode == NULL) || (mode != NULL && !strcmp(mode, "win")));
    const bool hbm = !win
        && ((max_phones > 64 * SSW_ALIGN_MAX_WAVES && lds > 160 * 1024)
            || (mode != NULL && !strcmp(mode, "hbm")));
    const int words_all = (max_phones + 63) / 64;
    /* which kernel (as below): the wave-per-word kernel -- and with `bt` its byte-token form */
    const bool take_mw = !win && !hbm && words_all <= SSW_ALIGN_MAX_WAVES
        && !(mode && (!strcmp(mode, "lds") || !strcmp(mode, "reg")))
        && (words_all > 4 || (int64_t)n_run * words_all <= 8192
            || (mode && (!strcmp(mode, "mw") || !strcmp(mode, "mwb"))));
    /* (a forced "mwb" still hands what it cannot replay to the full-token kernel: bt is false on
     * that second run; a forced "mw" never takes byte tokens) */
    const bool mwb = take_mw && bt && (mode == NULL || !strcmp(mode, "mwb"));
    *used_bt = mwb;
    int band_tokens = 0; /* tokens per frame the banded table budgets: 8 words of 64 phones */
    if ((hbm || win) && allow_band) {
        /* SSW_ALIGN_BAND_TOKENS (tests): small enough to overflow */
        band_tokens = m->kn.align_band_tokens > 0 ? m->kn.align_band_tokens : 8 * 192;
    }
    for (int i = 0; i < n_run; ++i) {
        const int u = utt_of(i);
        AlignUtt &U = utts[i];
        U.frame_off = frame_off[u];
        U.n_frames = frame_off[u + 1] - frame_off[u];
        U.phone_off = phone_off[u];
        U.n_phones = phone_off[u + 1] - phone_off[u];
        U.tok_off = tok_total;
        U.scr_off = cp != NULL ? cp->crow_off[(size_t)u] : (long long)U.frame_off * h->n_sen;
        U.scr_stride = cp != NULL ? cp->cstride[(size_t)u] : h->n_sen;
        U.pad_ = 0;
        if (U.n_phones < 1 || U.n_frames < 0) {
            ssw_set_error("utterance %d: %d phones, %d frames", u, U.n_phones, U.n_frames);
            return -1;
        }
        if (mwb) { /* bytes: [n_frames][64 words] tokens | [n_frames] int32 | [n_frames + 1] uint16 */
            const size_t tokb = align256((size_t)U.n_frames * 64 * words_all);
            tok_total += (long long)align256(tokb + 4 * (size_t)U.n_frames + 2 * ((size_t)U.n_frames + 1));
        } else
            tok_total += (long long)U.n_frames
                * (band_tokens ? std::min(U.n_phones * 3, band_tokens) : U.n_phones * 3);
    }
    for (int p = 0; p < total_phones; ++p)
        if (tmatid[p] < 0 || tmatid[p] >= h->tp_n_tmat) {
            ssw_set_error("phone %d: transition matrix %d out of range", p, tmatid[p]);
            return -1;
        }
    for (int i = 0; hbm && i < n_run; ++i)
        utts[i].ws_off = (long long)i * A_COUNT * (max_phones + 1);
    /* one grow-only device arena per model for the call's inputs, token stacks and results */
    WsLayout L;
    const size_t o_utts = L.out(sizeof(AlignUtt) * n_run);
    const size_t o_senid = L.out(sizeof(uint16_t) * 3 * (size_t)total_phones + 16);
    const size_t o_tmatid = L.out(sizeof(int16_t) * (size_t)total_phones + 16);
    const size_t o_sf = L.out(sizeof(int32_t) * (size_t)total_phones);
    const size_t o_ef = L.out(sizeof(int32_t) * (size_t)total_phones);
    const size_t o_status = L.out(sizeof(int32_t) * n_utts);
    const size_t o_state = L.out(sizeof(ssw_align_entry_t) * 3 * (size_t)total_phones);
    const size_t o_tok = L.out((mwb ? 1 : sizeof(int2)) * (size_t)(tok_total > 0 ? tok_total : 1));
    const size_t o_big = L.out(hbm ? sizeof(int) * (size_t)n_run * A_COUNT * (max_phones + 1) : 0);
    const size_t o_band = L.out(band_tokens ? sizeof(int) * (2 * (size_t)frame_off[n_utts] + 2 * (size_t)n_utts + 2) : 0);
    int rv = -1;
#define TRY(expr)                                                                            \
    if ((expr) != hipSuccess) {                                                              \
        ssw_set_error("%s failed: %s", #expr, hipGetErrorString(hipGetLastError()));         \
        goto out;                                                                            \
    }
    if (devbuf_reserve(m->align_ws, L.size(), "ssw_align_batch") < 0)
        goto out;
    {
    unsigned char *ws = m->align_ws.p;
    AlignUtt *d_utts = reinterpret_cast<AlignUtt *>(ws + o_utts);
    uint16_t *d_senid = reinterpret_cast<uint16_t *>(ws + o_senid);
    int16_t *d_tmatid = reinterpret_cast<int16_t *>(ws + o_tmatid);
    int32_t *d_sf = reinterpret_cast<int32_t *>(ws + o_sf);
    int32_t *d_ef = reinterpret_cast<int32_t *>(ws + o_ef);
    int32_t *d_status = reinterpret_cast<int32_t *>(ws + o_status);
    ssw_align_entry_t *d_state = reinterpret_cast<ssw_align_entry_t *>(ws + o_state);
    int2 *d_tok = reinterpret_cast<int2 *>(ws + o_tok);
    /* Round 5: everything the call uploads goes through ONE pinned staging slot (filled by the
     * host threads, then asynchronous copies on the caller's stream), and the state entries come
     * back the same way -- the runtime's pageable copies ran at ~10 GB/s and took 1.5 of the
     * 4.9 ms of a 2048-utterance call.  The workspace arena is laid out so that the uploaded
     * arrays are contiguous: one copy. */
    const size_t b_state = sizeof(ssw_align_entry_t) * 3 * (size_t)total_phones;
    /* SSW_ALIGN_STATE_OUT_ONLY drops the upload on the FIRST run of a batch only: a rerun of the
     * `only` utterances copies all of d_state back over state_io, which by then holds the first
     * run's results for everything else (zeros, or the restored entries, for the ones run again)
     * -- so a rerun uploads state_io like any in / out call (ADVICE r5: it used to clear d_state
     * and hand zeros back for every utterance the first run had aligned) */
    const bool state_out_only = m->align_state_out_only != 0 && only == NULL;
    {
        const size_t up_bytes = o_state - o_utts; /* utts | senid | tmatid | sf | ef | status */
        int slot = 0;
        unsigned char *hs = stage_acquire(m, up_bytes + (state_out_only ? 0 : b_state), &slot);
        if (hs == NULL)
            goto out;
        memcpy(hs + (o_utts - o_utts), utts.data(), sizeof(AlignUtt) * n_run);
        if (cp == NULL) /* (compact rows: the plan's per-state row indices are on the device) */
            host_copy_parallel(hs + (o_senid - o_utts), senid, sizeof(uint16_t) * 3 * (size_t)total_phones);
        memcpy(hs + (o_tmatid - o_utts), tmatid, sizeof(int16_t) * (size_t)total_phones);
        host_copy_parallel(hs + (o_sf - o_utts), sf, sizeof(int32_t) * (size_t)total_phones);
        host_copy_parallel(hs + (o_ef - o_utts), ef, sizeof(int32_t) * (size_t)total_phones);
        TRY(hipMemcpyAsync(ws + o_utts, hs, up_bytes, hipMemcpyHostToDevice, st));
        if (state_out_only) {
            TRY(hipMemsetAsync(d_state, 0, b_state, st));
        } else {
            host_copy_parallel(hs + up_bytes, state_io, b_state);
            TRY(hipMemcpyAsync(d_state, hs + up_bytes, b_state, hipMemcpyHostToDevice, st));
        }
        if (stage_release(m, slot, st) < 0)
            goto out;
    }
    {
        AlignParams A;
        A.senscr = d_senscr;
        A.utts = d_utts;
        A.senid = cp != NULL ? cp->d_cidx : d_senid;
        A.tmatid = d_tmatid;
        A.sf = d_sf;
        A.ef = d_ef;
        A.tp = m->d_tp;
        A.tokens = d_tok;
        A.btok = reinterpret_cast<uint8_t *>(d_tok);
        A.state_io = d_state;
        A.status = d_status;
        A.n_sen = h->n_sen;
        A.n_utts = n_run;
        A.max_phones = max_phones;
        A.big_ws = reinterpret_cast<int *>(ws + o_big);
        A.band_tokens = band_tokens;
        A.band_ws = reinterpret_cast<int *>(ws + o_band);
        const int words = (max_phones + 63) / 64;
        /* HMMs in registers: one wave per 64-phone word when the batch leaves SIMDs idle (the
         * usual case: a frame step is a short dependent chain), one wave per utterance for very
         * large batches; utterances beyond 1024 phones go through LDS */
        if (win) {
            /* window of 4 blocks (256 phones) unless told otherwise (2, 4, 8 or 16): with the
             * first pass's windows a frame has one or two active blocks, and four waves are one
             * per SIMD -- a second wave on a SIMD shares its issue port with the first (8 waves:
             * +14 % on the page) */
            const int want = m->kn.align_win_waves; /* SSW_ALIGN_WIN_WAVES */
            const int nwv = want >= 16 ? 16 : want >= 8 ? 8 : want >= 4 ? 4 : 2;
            hipLaunchKernelGGL(viterbi_align_win_kernel, dim3(n_run), dim3(64 * nwv), 0, st, A);
            TRY(hipGetLastError());
        } else if (hbm) {
            /* full table: only the walked words of a frame write their tokens, the rest must
             * read as -1; the banded table holds nothing but walked words */
            if (band_tokens == 0)
                TRY(hipMemsetAsync(d_tok, 0xff, sizeof(int2) * (size_t)(tok_total > 0 ? tok_total : 1), st));
            hipLaunchKernelGGL((viterbi_align_kernel<0, true>), dim3(n_run), dim3(64), 0, st, A);
            TRY(hipGetLastError());
        } else if (mwb) {
            m->align_stats[0] += n_run;
            hipLaunchKernelGGL(viterbi_align_mwb_kernel, dim3(n_run), dim3(64 * words), 0, st, A);
            TRY(hipGetLastError());
        } else if (take_mw) {
            hipLaunchKernelGGL(viterbi_align_mw_kernel, dim3(n_run), dim3(64 * words), 0, st, A);
            TRY(hipGetLastError());
        } else {
            const bool in_regs = words <= 4 && !(mode && !strcmp(mode, "lds"));
            void (*kern)(AlignParams) = words <= 1 ? viterbi_align_reg_kernel<1>
                : words <= 2                       ? viterbi_align_reg_kernel<2>
                : words <= 4                       ? viterbi_align_reg_kernel<4>
                : words <= 8                       ? viterbi_align_kernel<8>
                                                   : viterbi_align_kernel<0>;
            if (!in_regs && words <= 4)
                kern = viterbi_align_kernel<4>;
            if (!in_regs && lds > 64 * 1024)
                TRY(hipFuncSetAttribute((const void *)kern,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(n_run), dim3(64), in_regs ? 0 : lds, st, A);
            TRY(hipGetLastError());
        }
    }
    {
        /* results: status and state entries into pinned staging, then the caller's arrays */
        const size_t b_status = sizeof(int32_t) * (size_t)n_utts;
        int slot = 0;
        unsigned char *hs = stage_acquire(m, align256(b_status) + b_state, &slot);
        if (hs == NULL)
            goto out;
        unsigned char *h_state = hs + align256(b_status);
        TRY(hipMemcpyAsync(hs, d_status, sizeof(int32_t) * (size_t)(only == NULL ? n_utts : n_run),
                           hipMemcpyDeviceToHost, st));
        TRY(hipMemcpyAsync(h_state, d_state, b_state, hipMemcpyDeviceToHost, st));
        if (stage_release(m, slot, st) < 0)
            goto out;
        TRY(hipStreamSynchronize(st));
        const int32_t *got = reinterpret_cast<const int32_t *>(hs);
        if (only == NULL)
            memcpy(status, got, b_status);
        else
            for (int i = 0; i < n_run; ++i)
                status[only[i]] = got[i];
        host_copy_parallel(state_io, h_state, b_state);
    }
    rv = 0;
    }
out:
#undef TRY
    return rv;
}

/* [0] = utterances that went through the byte-token kernel, [1] = of those, the ones it handed to
 * the full-token kernel; running totals since the model was loaded */
extern "C" int
ssw_align_stats(ssw_model_t *m, int64_t stats[2])
{
    stats[0] = m->align_stats[0];
    stats[1] = m->align_stats[1];
    return 0;
}

extern "C" int
ssw_alignment_propagate(const ssw_align_entry_t *child, const int32_t *parent, int32_t n_child,
                        ssw_align_entry_t *parent_out, int32_t n_parent)
{
    int last = -1;
    for (int i = 0; i < n_child; ++i) {
        int p = parent[i];
        if (p < 0 || p >= n_parent) {
            ssw_set_error("child %d has parent %d of %d", i, p, n_parent);
            return -1;
        }
        if (p != last) { /* src/ps_alignment.c:326-330 */
            parent_out[p].start = child[i].start;
            parent_out[p].duration = 0;
            parent_out[p].score = 0;
        }
        parent_out[p].duration += child[i].duration;
        parent_out[p].score += child[i].score;
        last = p;
    }
    return 0;
}
