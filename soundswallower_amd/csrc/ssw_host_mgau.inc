/* ssw_host_mgau.inc -- host: mgau_t / mgaufuncs_t drop-in objects.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* scorer object: mgau_t / mgaufuncs_t drop-in                                          */
/* ---------------------------------------------------------------------------------- */
struct ssw_mgau_impl {
    ssw_mgau_s base; /* must be first: {vt, frame_idx} as in acmod.h:108-111 */
    ssw_model_s *m;
    int scorer;
    /* one-frame path: the reference's 2-deep history ring (src/ptm_mgau.c:425-448) */
    uint32_t *d_hist_cw[2];
    int4 *d_hist_sc[2];
    int *d_utt1;
    float *d_feat1;
    int16_t *d_out1;
    /* compallsen = no: the codebook activity of each history slot (mgau_active) travels as a
     * bit mask in the kernel arguments, the frame's senone list as a bit map in pinned,
     * device-mapped memory written with plain stores -- a blocking hipMemcpy each cost more than
     * the kernels of the frame */
    unsigned long long cb_mask[2][4];
    uint32_t *h_sen_bits, *dh_sen_bits; /* one bit per senone of the frame's delta list */
    unsigned *d_counter;      /* ptm_frame_kernel: ticket / barrier counter (only grows), best scores */
    unsigned counter_base;    /* the counter's value before the next call */
    int *h_done, *dh_done;    /* pinned: the sequence number of the last finished frame_eval */
    int seq;
    /* pinned, device-mapped staging of the one-frame call: the kernels read the feature row from
     * host memory and write the scores to it, so a frame costs two launches and one stream
     * synchronise instead of four blocking copies */
    float *h_feat1, *dh_feat1;
    int16_t *h_out1, *dh_out1;
    /* whole-utterance cache filled by ssw_mgau_prescore */
    std::vector<int16_t> cache;
    int cache_frames;
    int cache_gen; /* the model's MLLR generation the rows were scored at (mgau_cached) */
    /* the s2_semi scorer's ring of two slots (src/s2_semi_mgau.c:845-855), kept on the host: the
     * packed codeword order of every stream, and the whole row the slot's lists last gave */
    std::vector<uint32_t> sc_hist[2];
    std::vector<int16_t> sc_row[2];
};

static int mgau_frame_eval(ssw_mgau_t *mg, int16_t *senscr, uint8_t *senone_active,
                           int32_t n_senone_active, float **feat, int32_t frame,
                           int32_t compallsen);

static int mgau_transform(ssw_mgau_t *mg, void *mllr);
static void mgau_free(ssw_mgau_t *mg);

/* does ssw_mgau_prescore's cache hold `frame`, scored with the model's present parameters?  (rows
 * of before an ssw_model_apply_mllr -- through the vtable or not -- are not served) */
static inline bool
mgau_cached(const ssw_mgau_impl *g, int32_t frame)
{
    return frame < g->cache_frames && g->cache_gen == g->m->h->mllr_generation;
}

static ssw_mgaufuncs_t g_ptm_funcs = { "ptm", mgau_frame_eval, mgau_transform, mgau_free };

static int
mgau_alloc_pinned(ssw_mgau_impl *g)
{
    const ssw_host_model_t *h = g->m->h;
    g->h_feat1 = NULL;
    g->h_out1 = NULL;
    g->h_sen_bits = NULL;
    HIP_OK(hipHostMalloc((void **)&g->h_sen_bits, sizeof(uint32_t) * ((size_t)h->n_sen / 32 + 8),
                         hipHostMallocMapped));
    HIP_OK(hipHostGetDevicePointer((void **)&g->dh_sen_bits, g->h_sen_bits, 0));
    HIP_OK(hipHostMalloc((void **)&g->h_done, 64, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(hipHostGetDevicePointer((void **)&g->dh_done, g->h_done, 0));
    g->h_done[0] = 0;
    g->seq = 0;
    HIP_OK(hipMalloc((void **)&g->d_counter, 64));
    {
        const int init[3] = { 0, INT_MAX, INT_MAX }; /* counter, best score (two, by parity) */
        HIP_OK(hipMemcpy(g->d_counter, init, sizeof(init), hipMemcpyHostToDevice));
    }
    g->counter_base = 0u;
    HIP_OK(hipHostMalloc((void **)&g->h_feat1, sizeof(float) * SSW_MAX_FEAT * SSW_MAX_VECLEN,
                         hipHostMallocMapped));
    HIP_OK(hipHostMalloc((void **)&g->h_out1, sizeof(int16_t) * (size_t)h->n_sen + 32,
                         hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(hipHostGetDevicePointer((void **)&g->dh_feat1, g->h_feat1, 0));
    HIP_OK(hipHostGetDevicePointer((void **)&g->dh_out1, g->h_out1, 0));
    return 0;
}

static int
mgau_reset_device_hist(ssw_mgau_impl *g)
{
    std::vector<uint32_t> init((size_t)g->m->n_cbf, SSW_ORDER_RESET); /* cw = m */
    for (int i = 0; i < 2; ++i) {
        HIP_OK(hipMemcpy(g->d_hist_cw[i], init.data(), init.size() * 4, hipMemcpyHostToDevice));
        memset(g->cb_mask[i], 0xff, sizeof(g->cb_mask[i])); /* all codebooks active */
    }
    return 0;
}

extern "C" ssw_mgau_t *
ssw_ptm_mgau_init(ssw_model_t *m)
{
    if (check_scorer_shape(m, SSW_SCORER_PTM) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess) {
        ssw_set_error("hipSetDevice failed");
        return NULL;
    }
    ssw_mgau_impl *g = new ssw_mgau_impl();
    g->base.vt = &g_ptm_funcs;
    g->base.frame_idx = 0;
    g->m = m;
    g->scorer = SSW_SCORER_PTM;
    g->cache_frames = 0;
    g->d_utt1 = NULL;
    g->d_feat1 = NULL;
    g->d_out1 = NULL;
    for (int i = 0; i < 2; ++i) {
        g->d_hist_cw[i] = NULL;
        g->d_hist_sc[i] = NULL;
    }
    bool ok = true;
    for (int i = 0; i < 2 && ok; ++i)
        ok = dev_alloc(&g->d_hist_cw[i], (size_t)m->n_cbf) == 0
            && dev_alloc(&g->d_hist_sc[i], (size_t)m->n_cbf) == 0;
    ok = ok && dev_alloc(&g->d_utt1, 2) == 0 && dev_alloc(&g->d_feat1, (size_t)m->h->veclen_total) == 0
        && dev_alloc(&g->d_out1, (size_t)m->h->n_sen) == 0;
    /* (every codebook starts active, src/ptm_mgau.c:716-718: mgau_reset_device_hist below) */
    int one[2] = { 0, 1 };
    ok = ok && hipMemcpy(g->d_utt1, one, sizeof(one), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && mgau_alloc_pinned(g) == 0;
    ok = ok && mgau_reset_device_hist(g) == 0;
    if (!ok) {
        mgau_free(&g->base);
        return NULL;
    }
    return &g->base;
}

static ssw_mgaufuncs_t g_ms_funcs = { "ms", mgau_frame_eval, mgau_transform, mgau_free };

/* ms_mgau_init(acmod_t *) (src/ms_mgau.c:165): needs a model loaded with a mixture_weights file */
extern "C" ssw_mgau_t *
ssw_ms_mgau_init(ssw_model_t *m)
{
    if (check_scorer_shape(m, SSW_SCORER_MS) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess) {
        ssw_set_error("hipSetDevice failed");
        return NULL;
    }
    ssw_mgau_impl *g = new ssw_mgau_impl();
    g->base.vt = &g_ms_funcs;
    g->base.frame_idx = 0;
    g->m = m;
    g->scorer = SSW_SCORER_MS;
    g->cache_frames = 0;
    g->d_utt1 = NULL;
    g->d_feat1 = NULL;
    g->d_out1 = NULL;
    for (int i = 0; i < 2; ++i) {
        g->d_hist_cw[i] = NULL;
        g->d_hist_sc[i] = NULL;
    }
    if (dev_alloc(&g->d_feat1, (size_t)m->h->veclen_total) < 0
        || dev_alloc(&g->d_out1, (size_t)m->h->n_sen) < 0) {
        mgau_free(&g->base);
        return NULL;
    }
    return &g->base;
}

static void
semi_mgau_reset(ssw_mgau_impl *g)
{
    for (int i = 0; i < 2; ++i) {
        g->sc_hist[i].assign((size_t)g->m->n_cbf, SSW_ORDER_RESET); /* codeword k (:993-1002) */
        g->sc_row[i].assign((size_t)g->m->h->n_sen, 0);
    }
}

static ssw_mgaufuncs_t g_s2_semi_funcs = { "s2_semi", mgau_frame_eval, mgau_transform, mgau_free };

/* s2_semi_mgau_init(acmod_t *) (src/s2_semi_mgau.c:1014): a single-codebook model.  frame_eval
 * scores a frame that acmod has not scored yet (frame >= frame_idx) as a batch of one, from the
 * other slot's order, and keeps the row; an earlier frame gets its slot's row again, as the
 * reference makes it again from the slot's lists.  With compallsen = 0 the listed senones (the
 * delta list's bridge entries included) get their values and every other one 0: the Gaussians and
 * the normalisation do not depend on the list (:841-872). */
extern "C" ssw_mgau_t *
ssw_s2_semi_mgau_init(ssw_model_t *m)
{
    if (check_scorer_shape(m, SSW_SCORER_S2_SEMI) < 0)
        return NULL;
    if (hipSetDevice(m->device) != hipSuccess) {
        ssw_set_error("hipSetDevice failed");
        return NULL;
    }
    ssw_mgau_impl *g = new ssw_mgau_impl();
    g->base.vt = &g_s2_semi_funcs;
    g->base.frame_idx = 0;
    g->m = m;
    g->scorer = SSW_SCORER_S2_SEMI;
    g->cache_frames = 0;
    if (dev_alloc(&g->d_feat1, (size_t)m->h->veclen_total) < 0
        || dev_alloc(&g->d_out1, (size_t)m->h->n_sen) < 0) {
        mgau_free(&g->base);
        return NULL;
    }
    semi_mgau_reset(g);
    return &g->base;
}

static int
semi_mgau_frame_eval(ssw_mgau_impl *g, int16_t *senscr, const uint8_t *senone_active,
                     int32_t n_senone_active, float **feat, int32_t frame, int32_t compallsen)
{
    ssw_model_s *m = g->m;
    const ssw_host_model_t *h = m->h;
    const int slot = frame % 2;
    const int16_t *row = g->sc_row[slot].data();
    if (mgau_cached(g, frame)) /* ssw_mgau_prescore */
        row = g->cache.data() + (size_t)frame * h->n_sen;
    else if (frame >= g->base.frame_idx) {
        std::vector<float> x((size_t)h->veclen_total);
        for (int f = 0; f < h->n_feat; ++f)
            memcpy(x.data() + h->featoff[f], feat[f], sizeof(float) * h->veclen[f]);
        const int32_t off[2] = { 0, 1 };
        HIP_OK(hipMemcpy(g->d_feat1, x.data(), sizeof(float) * x.size(), hipMemcpyHostToDevice));
        ScoreReq R{};
        R.scorer = SSW_SCORER_S2_SEMI;
        R.d_feats = g->d_feat1;
        R.n_frames = 1;
        R.utt_off = off;
        R.n_utts = 1;
        R.d_out = g->d_out1;
        R.carry_in = g->sc_hist[slot ^ 1].data();
        R.carry_out = g->sc_hist[slot].data();
        R.frame_base = frame; /* (the frame's number decides whether a ds > 1 model scans the codebook) */
        if (score_batch_impl(m, R) < 0)
            return -1;
        HIP_OK(hipMemcpy(g->sc_row[slot].data(), g->d_out1, sizeof(int16_t) * h->n_sen,
                         hipMemcpyDeviceToHost));
    }
    if (compallsen) {
        memcpy(senscr, row, sizeof(int16_t) * h->n_sen);
        return 0;
    }
    memset(senscr, 0, sizeof(int16_t) * h->n_sen); /* (:841) */
    int at = 0;
    for (int32_t i = 0; i < n_senone_active; ++i) {
        at += senone_active[i];
        if (at >= h->n_sen) {
            ssw_set_error("active list runs past the last senone (%d >= %d)", at, h->n_sen);
            return -1;
        }
        senscr[at] = row[at];
    }
    return 0;
}

extern "C" void
ssw_mgau_reset_hist(ssw_mgau_t *mg)
{
    ssw_mgau_impl *g = reinterpret_cast<ssw_mgau_impl *>(mg);
    (void)hipSetDevice(g->m->device);
    if (g->scorer == SSW_SCORER_PTM)
        (void)mgau_reset_device_hist(g);
    if (g->scorer == SSW_SCORER_S2_SEMI)
        semi_mgau_reset(g);
    g->cache_frames = 0;
}

extern "C" int
ssw_mgau_prescore(ssw_mgau_t *mg, const float *feats, int32_t n_frames)
{
    ssw_mgau_impl *g = reinterpret_cast<ssw_mgau_impl *>(mg);
    g->cache_frames = 0;
    if (n_frames <= 0)
        return 0;
    g->cache.resize((size_t)n_frames * g->m->h->n_sen);
    int32_t off[2] = { 0, n_frames };
    if (ssw_score_batch_host(g->m, g->scorer, feats, n_frames, off, 1, g->cache.data()) < 0)
        return -1;
    g->cache_frames = n_frames;
    g->cache_gen = g->m->h->mllr_generation;
    return 0;
}

/* uint8 delta list (acmod_flags2list, src/acmod.c:947-999) -> per-senone and per-codebook
 * activity, exactly as ptm_mgau_calc_cb_active / ms_cont_mgau_frame_eval walk it */
static int
decode_active(const ssw_host_model_t *h, const uint8_t *list, int32_t n, std::vector<uint8_t> &sen,
              std::vector<uint8_t> &cb)
{
    sen.assign((size_t)h->n_sen, 0);
    cb.assign((size_t)h->n_cb, 0);
    int last = 0;
    for (int32_t i = 0; i < n; ++i) {
        int s = list[i] + last;
        if (s >= h->n_sen) {
            ssw_set_error("active list runs past the last senone (%d >= %d)", s, h->n_sen);
            return -1;
        }
        sen[s] = 1;
        cb[h->sen2cb[s]] = 1;
        last = s;
    }
    return 0;
}

/* frame_eval slot of mgaufuncs_t (acmod.h:96-102); semantics of ptm_mgau_frame_eval
 * (src/ptm_mgau.c:408-454) and ms_cont_mgau_frame_eval (src/ms_mgau.c:278-368), both for
 * compallsen = yes and for an active-senone list. */
static int
mgau_frame_eval(ssw_mgau_t *mg, int16_t *senscr, uint8_t *senone_active,
                int32_t n_senone_active, float **feat, int32_t frame, int32_t compallsen)
{
    ssw_mgau_impl *g = reinterpret_cast<ssw_mgau_impl *>(mg);
    ssw_model_s *m = g->m;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    if (frame < 0) {
        ssw_set_error("negative frame");
        return -1;
    }
    if (!compallsen && (senone_active == NULL || n_senone_active < 0)) {
        ssw_set_error("compallsen=no needs the active senone list");
        return -1;
    }
    if (compallsen && mgau_cached(g, frame)) {
        memcpy(senscr, g->cache.data() + (size_t)frame * h->n_sen, sizeof(int16_t) * h->n_sen);
        return 0;
    }
    HIP_OK(hipSetDevice(m->device));
    if (g->scorer == SSW_SCORER_S2_SEMI)
        return semi_mgau_frame_eval(g, senscr, senone_active, n_senone_active, feat, frame,
                                    compallsen);
    std::vector<uint8_t> sen_act, cb_act; /* (the ms path's per-senone view of the list) */
    if (!compallsen && g->scorer == SSW_SCORER_MS
        && decode_active(h, senone_active, n_senone_active, sen_act, cb_act) < 0)
        return -1;
    float row[SSW_MAX_FEAT * SSW_CONT_MAX_VECLEN]; /* (the widest model the loader accepts) */
    for (int f = 0; f < h->n_feat; ++f)
        memcpy(row + h->featoff[f], feat[f], sizeof(float) * h->veclen[f]);

    if (g->scorer == SSW_SCORER_MS) { /* history-free: one frame is a batch of one */
        int32_t off[2] = { 0, 1 };
        HIP_OK(hipMemcpy(g->d_feat1, row, sizeof(float) * h->veclen_total, hipMemcpyHostToDevice));
        m->ms_raw = compallsen ? 0 : 1;
        int rv = ssw_score_batch(m, SSW_SCORER_MS, g->d_feat1, 1, off, 1, g->d_out1, NULL);
        m->ms_raw = 0;
        if (rv < 0)
            return -1;
        if (compallsen) {
            HIP_OK(hipMemcpy(senscr, g->d_out1, sizeof(int16_t) * h->n_sen, hipMemcpyDeviceToHost));
            return 0;
        }
        /* only active senones are written; they are normalised by the best active one
         * (src/ms_mgau.c:342-364).  Densities of inactive codebooks are simply not used. */
        std::vector<int16_t> raw((size_t)h->n_sen);
        HIP_OK(hipMemcpy(raw.data(), g->d_out1, sizeof(int16_t) * h->n_sen, hipMemcpyDeviceToHost));
        int best = INT_MAX;
        for (int s = 0; s < h->n_sen; ++s)
            if (sen_act[s] && raw[s] < best)
                best = raw[s];
        for (int s = 0; s < h->n_sen; ++s)
            if (sen_act[s])
                senscr[s] = (int16_t)clamp_i16(raw[s] - best);
        return 0;
    }

    const int slot = frame % 2;
    FrameFusedParams Q;
    memset(&Q, 0, sizeof(Q));
    Q.run_topn = frame >= g->base.frame_idx;
    /* the uint8 delta list (acmod_flags2list, src/acmod.c:947-999) -> a bit per senone, where
     * the kernel reads it, and a bit per codebook (ptm_mgau_calc_cb_active, src/ptm_mgau.c:
     * 297-321) */
    unsigned long long cbm[4] = { ~0ull, ~0ull, ~0ull, ~0ull };
    if (!compallsen) {
        const int n_words = h->n_sen / 32 + 1;
        memset(g->h_sen_bits, 0, sizeof(uint32_t) * (size_t)n_words);
        memset(cbm, 0, sizeof(cbm));
        int at = 0;
        for (int32_t i = 0; i < n_senone_active; ++i) {
            at += senone_active[i];
            if (at >= h->n_sen) {
                ssw_set_error("active list runs past the last senone (%d >= %d)", at, h->n_sen);
                return -1;
            }
            g->h_sen_bits[at >> 5] |= 1u << (at & 31);
            const int c = h->sen2cb[at];
            cbm[c >> 6] |= 1ull << (c & 63);
        }
    }
    if (Q.run_topn) {
        memcpy(g->h_feat1, row, sizeof(float) * h->veclen_total);
        memcpy(g->cb_mask[slot], cbm, sizeof(cbm)); /* the slot's mgau_active */
        fill_chain_params(m, Q.C, g->dh_feat1);
        Q.C.utt_off = g->d_utt1;
        Q.C.n_utts = 1;
        Q.C.carry_pk = g->d_hist_cw[slot ^ 1]; /* lastf, src/ptm_mgau.c:435-441 */
        Q.C.cb_active = NULL;                  /* (the mask below) */
        Q.C.topn_cw = g->d_hist_cw[slot];
        Q.C.topn_sc = g->d_hist_sc[slot];
        Q.C.frame_base = frame;
    }
    {
        SenoneFrameParams &F = Q.S;
        F.topn_cw = g->d_hist_cw[slot];
        F.topn_sc = g->d_hist_sc[slot];
        F.mixw = m->d_mixw;
        F.quad_cb = m->d_quad_cb;
        F.logadd8 = m->d_logadd8;
        memcpy(F.cb_mask, g->cb_mask[slot], sizeof(F.cb_mask));
        F.sen_bits = compallsen ? NULL : g->dh_sen_bits;
        F.slot_sen = m->d_slot_sen;
        F.out = g->dh_out1;
        F.raw = g->d_out1;
        F.n_cb = h->n_cb;
        F.n_feat = h->n_feat;
        F.n_density = h->n_density;
        F.n_sen = h->n_sen;
        F.slot_stride = m->slot_stride;
        F.n_quads = m->n_quads;
    }
    /* Three launches, one after the other on the stream: the exact top-N step (a wave per
     * codebook x stream), the senone combine (a thread per slot; the frame's best by an atomic
     * minimum), score - best to pinned memory (8 senones per thread) and, behind them, the call's
     * sequence number, on which the host spins -- a stream synchronise costs more than the
     * kernels.  SSW_FRAME_FUSED=1: the same as ONE launch with device-wide barriers (slower). */
    const int g_topn = (m->n_cbf + 3) / 4, g_slot = (m->n_quads * 4 + 255) / 256,
              g_out = ((h->n_sen + 7) / 8 + 255) / 256;
    Q.counter = g->d_counter;
    Q.gbest = reinterpret_cast<int *>(g->d_counter + 1);
    Q.base = g->counter_base;
    Q.done = g->dh_done;
    Q.seq = ++g->seq;
    const size_t lds = 8 * (size_t)m->n_cbf;
    refresh_knobs(m);
    if (m->kn.frame_fused) { /* SSW_FRAME_FUSED */
        const int n_groups = std::max(g_topn, std::max(g_slot, g_out));
        if (n_groups > 512) { /* the kernel's barrier needs every group resident at once */
            ssw_set_error("frame_eval: %d codebook x stream pairs / %d senones are more than the "
                          "one-launch kernel's grid may hold", m->n_cbf, h->n_sen);
            return -1;
        }
        g->counter_base += 3u * (unsigned)n_groups;
        hipLaunchKernelGGL(ptm_frame_kernel<0>, dim3(n_groups), dim3(256), lds, 0, Q);
    } else {
        g->counter_base += (unsigned)g_out;
        if (Q.run_topn)
            hipLaunchKernelGGL(ptm_frame_kernel<1>, dim3(g_topn), dim3(256), 0, 0, Q);
        hipLaunchKernelGGL(ptm_frame_kernel<2>, dim3(g_slot), dim3(256), lds, 0, Q);
        hipLaunchKernelGGL(ptm_frame_kernel<3>, dim3(g_out), dim3(256), 0, 0, Q);
    }
    HIP_OK(hipGetLastError());
    {
        volatile int *done = g->h_done;
        long spins = 0;
        while (__atomic_load_n(done, __ATOMIC_ACQUIRE) != Q.seq)
            if (++spins > 20000000L) { /* ~ tens of ms */
                HIP_OK(hipStreamSynchronize(0));
                if (__atomic_load_n(done, __ATOMIC_ACQUIRE) != Q.seq) {
                    const int init[3] = { 0, INT_MAX, INT_MAX }; /* start the counter afresh */
                    (void)hipMemcpy(g->d_counter, init, sizeof(init), hipMemcpyHostToDevice);
                    g->counter_base = 0u;
                    ssw_set_error("frame_eval: the kernel ended without reporting frame %d", frame);
                    return -1;
                }
                break;
            }
    }
    memcpy(senscr, g->h_out1, sizeof(int16_t) * h->n_sen);
    return 0;
}

static int
mgau_transform(ssw_mgau_t *mg, void *mllr)
{
    ssw_mgau_impl *g = reinterpret_cast<ssw_mgau_impl *>(mg);
    if (mllr == NULL) { /* (acmod_update_mllr never passes one) */
        ssw_set_error("transform: no MLLR transform given");
        return -1;
    }
    /* ptm_mgau_mllr_transform, ms_mgau_mllr_transform, s2_semi_mgau_mllr_transform: all three
     * are gauden_mllr_transform on the scorer's Gaussians; the top-N history stays as it is */
    if (ssw_model_apply_mllr(g->m, static_cast<const ssw_mllr_t *>(mllr)) < 0)
        return -1;
    g->cache_frames = 0; /* ssw_mgau_prescore's rows are the old parameters' */
    return 0;
}

static void
mgau_free(ssw_mgau_t *mg)
{
    ssw_mgau_impl *g = reinterpret_cast<ssw_mgau_impl *>(mg);
    if (g == NULL)
        return;
    (void)hipStreamSynchronize(0); /* the last frame's kernel may still be retiring */
    for (int i = 0; i < 2; ++i) {
        (void)hipFree(g->d_hist_cw[i]);
        (void)hipFree(g->d_hist_sc[i]);
    }
    (void)hipFree(g->d_utt1);
    (void)hipFree(g->d_feat1);
    (void)hipFree(g->d_out1);
    (void)hipHostFree(g->h_feat1);
    (void)hipHostFree(g->h_out1);
    if (g->h_sen_bits)
        (void)hipHostFree(g->h_sen_bits);
    if (g->h_done)
        (void)hipHostFree(g->h_done);
    (void)hipFree(g->d_counter);
    delete g;
}
