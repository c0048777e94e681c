/* ssw_host_fe.inc -- host: ssw_fe_batch(_ex, _f32), ssw_fe_frame_count(_ex), ssw_model_fe_config.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* MFCC front end (SURVEY 2 row 19, 8(f)): PCM -> cepstra for a batch                    */
/* ---------------------------------------------------------------------------------- */
extern "C" int
ssw_model_fe_config(const ssw_model_t *m, ssw_fe_config_t *out)
{
    if (m == NULL || out == NULL) {
        ssw_set_error("bad arguments to ssw_model_fe_config");
        return -1;
    }
    *out = m->h->fe;
    return 0;
}

extern "C" int64_t
ssw_fe_frame_count(const ssw_model_t *m, int64_t n_samples)
{
    if (m == NULL || n_samples < 0) {
        ssw_set_error("bad arguments to ssw_fe_frame_count");
        return -1;
    }
    return ssw_fe_frames_of(n_samples);
}

extern "C" int64_t
ssw_fe_frame_count_ex(const ssw_model_t *m, const ssw_fe_config_t *cfg, double samprate,
                      int64_t n_samples)
{
    if (m == NULL || n_samples < 0) {
        ssw_set_error("bad arguments to ssw_fe_frame_count_ex");
        return -1;
    }
    if (cfg == NULL && m->h->fe_err[0]) {
        ssw_set_error("ssw_fe_frame_count_ex: the model's feat_params.json cannot be used: %s",
                      m->h->fe_err);
        return -1;
    }
    ssw_fe_framing_t f;
    if (ssw_fe_framing(cfg != NULL ? cfg : &m->h->fe, samprate, &f) < 0)
        return -1;
    return ssw_fe_frames_at(&f, n_samples);
}

/* the tables for configuration c on the host when the device copy was built for another one
 * (NULL and *ok when it is current) */
static std::unique_ptr<ssw_fe_tables_t>
fe_tables_if_new(const ssw_model_s *m, const ssw_fe_config_t *c, ssw_fe_config_t *key, bool *ok)
{
    *key = *c;
    key->from_file = 0;
    *ok = true;
    if (m->d_fe_tab != NULL && memcmp(key, &m->fe_tab_cfg, sizeof(*key)) == 0)
        return nullptr;
    std::unique_ptr<ssw_fe_tables_t> t(new ssw_fe_tables_t());
    if (ssw_fe_tables_build(c, t.get()) < 0) {
        *ok = false;
        return nullptr;
    }
    return t;
}

static int
fe_tables_upload(ssw_model_s *m, const ssw_fe_tables_t *t, const ssw_fe_config_t *key)
{
    if (m->d_fe_tab == NULL)
        HIP_OK(hipMalloc((void **)&m->d_fe_tab, sizeof(ssw_fe_tables_t)));
    /* (every front-end call is synchronous: no launch still reads the old tables) */
    HIP_OK(hipMemcpy(m->d_fe_tab, t, sizeof(ssw_fe_tables_t), hipMemcpyHostToDevice));
    m->fe_tab_cfg = *key;
    m->fe_nfilt = t->nfilt;
    m->fe_noise = t->remove_noise;
    return 0;
}

/* one distinct (samprate, nfft) of a batch: its framing, its table block on the host until it
 * is uploaded (NULL when the model already holds it) and on the device */
struct FeRate {
    ssw_fe_framing_t fr;
    std::string key;
    std::unique_ptr<ssw_fe_rate_t, void (*)(void *)> host{nullptr, free};
    ssw_fe_rate_t *dev = nullptr;
};

/* key: the bytes of the configuration (ssw_fe_config_t, or ssw_fe_s for ssw_fe_batch_any's own
 * tables, which differ in length) */
static std::string
fe_rate_key(const std::string &key, const ssw_fe_framing_t *fr)
{
    return key + std::string((const char *)fr, sizeof(*fr));
}

/* the rate blocks the model does not hold yet, on the device; a model that has gathered more
 * than 64 first drops those this batch does not use (every front-end call is synchronous: no
 * launch still reads them) */
static int
fe_rates_upload(ssw_model_s *m, std::vector<FeRate> &rates)
{
    size_t fresh = 0;
    for (FeRate &r : rates)
        fresh += r.host != nullptr;
    if (fresh && m->fe_rate_tab->size() + fresh > 64) {
        std::set<std::string> used;
        for (FeRate &r : rates)
            used.insert(r.key);
        for (auto it = m->fe_rate_tab->begin(); it != m->fe_rate_tab->end();) {
            if (used.count(it->first)) {
                ++it;
            } else {
                (void)hipFree(it->second);
                it = m->fe_rate_tab->erase(it);
            }
        }
    }
    for (FeRate &r : rates) {
        if (r.host == nullptr)
            continue;
        ssw_fe_rate_t *d = NULL;
        HIP_OK(hipMalloc((void **)&d, (size_t)r.host->bytes));
        if (hipMemcpy(d, r.host.get(), (size_t)r.host->bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            ssw_set_error("front end: cannot upload a rate table");
            return -1;
        }
        (*m->fe_rate_tab)[r.key] = d;
        r.dev = d;
    }
    return 0;
}

/* ssw_fe_batch, ssw_fe_batch_ex, ssw_fe_batch_f32 and ssw_fe_batch_any: every utterance at
 * samprate[u] (NULL: c->samprate; ex = 0: ssw_fe_batch's checks, which allow 16 kHz only); d_pcm
 * holds float32 samples when f32, int16 otherwise.  any: NULL, or the resolved configuration
 * whose settings the kernels of ssw_k8_fe_any.inc compute (cfg is then its cfg, checked when it
 * was resolved) */
static int
fe_batch(ssw_model_t *m, const ssw_fe_config_t *cfg, const void *d_pcm, const int64_t *samp_off,
         const double *samprate, int32_t n_utts, float *d_cep, int32_t *frame_off_out,
         void *stream, bool ex, bool f32, const char *who, const ssw_fe_s *any = nullptr)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to %s", who);
        return -1;
    }
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    if (n_utts < 0 || samp_off == NULL || frame_off_out == NULL || samp_off[0] != 0) {
        ssw_set_error("bad arguments to %s", who);
        return -1;
    }
    if (cfg == NULL && m->h->fe_err[0]) {
        ssw_set_error("%s: the model's feat_params.json cannot be used: %s", who, m->h->fe_err);
        return -1;
    }
    const ssw_fe_config_t *c = cfg != NULL ? cfg : &m->h->fe;
    if (any == nullptr && (ex ? ssw_fe_config_check_ex(c) : ssw_fe_config_check(c)) < 0)
        return -1;
    ssw_fe_config_t key;
    bool ok = true;
    std::unique_ptr<ssw_fe_tables_t> fresh;
    std::unique_ptr<ssw_fe_any_tables_t> fresh_any;
    if (any == nullptr) {
        fresh = fe_tables_if_new(m, c, &key, &ok);
    } else if (m->d_fe_any_tab == NULL || memcmp(any, &m->fe_any_key, sizeof(*any)) != 0) {
        fresh_any.reset(new ssw_fe_any_tables_t());
        ssw_fe_any_tables_build(any, fresh_any.get());
    }
    if (!ok)
        return -1;
    const std::string key_bytes = any != nullptr ? std::string((const char *)any, sizeof(*any))
                                                 : std::string((const char *)&key, sizeof(key));
    /* every utterance's framing, and the distinct (samprate, nfft) of the batch, before anything
     * is written */
    if (m->fe_rate_tab == nullptr)
        m->fe_rate_tab = new std::map<std::string, ssw_fe_rate_t *>();
    std::vector<FeRate> rates;
    std::vector<int> rate_of((size_t)n_utts);
    std::vector<int32_t> foff((size_t)n_utts + 1);
    int64_t total = 0;
    for (int32_t u = 0; u < n_utts; ++u) {
        const int64_t n = samp_off[u + 1] - samp_off[u];
        if (n < 0) {
            ssw_set_error("%s: samp_off decreases at utterance %d", who, u);
            return -1;
        }
        ssw_fe_framing_t fr;
        if (ssw_fe_framing(c, samprate != NULL ? samprate[u] : c->samprate, &fr) < 0) {
            if (samprate != NULL) {
                std::string why = ssw_last_error();
                ssw_set_error("%s: utterance %d: %s", who, u, why.c_str());
            }
            return -1;
        }
        size_t r = 0;
        while (r < rates.size() && memcmp(&rates[r].fr, &fr, sizeof(fr)) != 0)
            ++r;
        if (r == rates.size()) {
            rates.emplace_back();
            rates[r].fr = fr;
            rates[r].key = fe_rate_key(key_bytes, &fr);
            auto hit = m->fe_rate_tab->find(rates[r].key);
            if (hit != m->fe_rate_tab->end()) {
                rates[r].dev = hit->second;
            } else {
                rates[r].host.reset(any != nullptr ? ssw_fe_any_rate_build(any, &fr)
                                                   : ssw_fe_rate_build(c, &fr, ex));
                if (rates[r].host == nullptr)
                    return -1;
            }
        }
        rate_of[u] = (int)r;
        total += ssw_fe_frames_at(&fr, n);
        if (total > INT32_MAX) {
            ssw_set_error("%s: more than 2^31 - 1 frames in one batch", who);
            return -1;
        }
        foff[u + 1] = (int32_t)total;
    }
    memcpy(frame_off_out, foff.data(), sizeof(int32_t) * ((size_t)n_utts + 1));
    if (total == 0)
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (d_pcm == NULL || d_cep == NULL) {
        ssw_set_error("bad arguments to %s", who);
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    if (fresh && fe_tables_upload(m, fresh.get(), &key) < 0)
        return -1;
    if (fresh_any) {
        if (m->d_fe_any_tab == NULL)
            HIP_OK(hipMalloc((void **)&m->d_fe_any_tab, sizeof(ssw_fe_any_tables_t)));
        HIP_OK(hipMemcpy(m->d_fe_any_tab, fresh_any.get(), sizeof(ssw_fe_any_tables_t),
                         hipMemcpyHostToDevice));
        m->fe_any_key = *any;
    }
    if (fe_rates_upload(m, rates) < 0)
        return -1;
    /* the utterance records, the frame offsets, and per FFT size present the group's
     * utterances and frame prefix (one spectrum launch each) */
    std::vector<FeUtt> utt((size_t)n_utts);
    int grp_frames[SSW_FE_MAX_LOG2N + 1] = {0}, grp_n[SSW_FE_MAX_LOG2N + 1] = {0};
    /* remove_dc: a launch sums its frames in any order only where that is exact at every rate
     * it holds (ssw_fe_dc_sum_exact) */
    int grp_dc[SSW_FE_MAX_LOG2N + 1];
    for (int o = 0; o <= SSW_FE_MAX_LOG2N; ++o)
        grp_dc[o] = any != nullptr && any->cfg.remove_dc ? SSW_FE_DC_ANY_ORDER : SSW_FE_DC_NONE;
    for (int32_t u = 0; u < n_utts; ++u) {
        const FeRate &r = rates[(size_t)rate_of[u]];
        utt[u].start = samp_off[u];
        utt[u].n = samp_off[u + 1] - samp_off[u];
        utt[u].rate = r.dev;
        utt[u].f0 = foff[u];
        utt[u].shift = r.fr.frame_shift;
        utt[u].size = r.fr.frame_size;
        utt[u].pad = 0;
        ++grp_n[r.fr.fft_order];
        if (grp_dc[r.fr.fft_order] == SSW_FE_DC_ANY_ORDER
            && !ssw_fe_dc_sum_exact((float)any->cfg.alpha, r.fr.frame_size, f32))
            grp_dc[r.fr.fft_order] = SSW_FE_DC_IN_ORDER;
    }
    std::vector<int> grp_utt((size_t)n_utts), grp_off((size_t)n_utts + SSW_FE_MAX_LOG2N + 1);
    int grp_at[SSW_FE_MAX_LOG2N + 1], off_at[SSW_FE_MAX_LOG2N + 1];
    for (int o = 0, a = 0, b = 0; o <= SSW_FE_MAX_LOG2N; ++o) {
        grp_at[o] = a;
        off_at[o] = b;
        a += grp_n[o];
        b += grp_n[o] ? grp_n[o] + 1 : 0;
    }
    {
        int fill[SSW_FE_MAX_LOG2N + 1] = {0};
        for (int32_t u = 0; u < n_utts; ++u) {
            const int o = rates[(size_t)rate_of[u]].fr.fft_order, k = fill[o]++;
            grp_utt[(size_t)grp_at[o] + k] = u;
            grp_off[(size_t)off_at[o] + k + 1] = grp_off[(size_t)off_at[o] + k] + (foff[u + 1] - foff[u]);
        }
        for (int o = 0; o <= SSW_FE_MAX_LOG2N; ++o)
            grp_frames[o] = grp_n[o] ? grp_off[(size_t)off_at[o] + grp_n[o]] : 0;
    }
    const int n_frames = (int)total, nfilt = any != nullptr ? any->cfg.nfilt : m->fe_nfilt;
    const bool noise = any != nullptr ? any->cfg.remove_noise != 0 : m->fe_noise != 0;
    /* grow-only workspace: records, offsets, groups, then the mel spectra */
    const size_t utt_bytes = sizeof(FeUtt) * (size_t)n_utts;
    const size_t int_bytes = sizeof(int) * (grp_utt.size() + grp_off.size() + (size_t)n_utts + 1);
    const size_t off_bytes = align256(utt_bytes + int_bytes);
    const size_t ws = off_bytes + (size_t)n_frames * nfilt * sizeof(double);
    if (devbuf_reserve(m->fe_ws, ws, who) < 0)
        return -1;
    std::vector<unsigned char> stage(utt_bytes + int_bytes);
    {
        unsigned char *p = stage.data();
        memcpy(p, utt.data(), utt_bytes);
        p += utt_bytes;
        memcpy(p, foff.data(), sizeof(int) * foff.size());
        p += sizeof(int) * foff.size();
        memcpy(p, grp_utt.data(), sizeof(int) * grp_utt.size());
        p += sizeof(int) * grp_utt.size();
        memcpy(p, grp_off.data(), sizeof(int) * grp_off.size());
    }
    FeParams F;
    F.pcm = d_pcm;
    F.utt = (const FeUtt *)m->fe_ws.p;
    F.frame_off = (const int *)(m->fe_ws.p + utt_bytes);
    const int *d_grp_utt = F.frame_off + n_utts + 1;
    const int *d_grp_off = d_grp_utt + n_utts;
    /* (fe_noise_kernel reads nfilt alone, which both table blocks begin with) */
    F.tab = any != nullptr ? (const ssw_fe_tables_t *)m->d_fe_any_tab : m->d_fe_tab;
    F.mfspec = (double *)(m->fe_ws.p + off_bytes);
    F.cep = d_cep;
    F.grp_utt = F.grp_off = nullptr; /* (set per spectrum launch) */
    F.n_grp = F.n_grp_frames = 0;
    F.n_utts = n_utts;
    F.n_frames = n_frames;
    if (m->sw.timing && !m->fe_ev_ready) {
        for (int i = 0; i < 4; ++i)
            HIP_OK(hipEventCreate(&m->fe_ev[i]));
        m->fe_ev_ready = 1;
    }
    const bool timed = m->sw.timing && m->fe_ev_ready;
    hipError_t e = hipMemcpyAsync(m->fe_ws.p, stage.data(), stage.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[0], st);
    for (int o = SSW_FE_MIN_LOG2N; o <= SSW_FE_MAX_LOG2N && e == hipSuccess; ++o) {
        if (grp_frames[o] == 0)
            continue;
        FeParams G = F;
        G.grp_utt = d_grp_utt + grp_at[o];
        G.grp_off = d_grp_off + off_at[o];
        G.n_grp = grp_n[o];
        G.n_grp_frames = grp_frames[o];
        if (any == nullptr && !f32) switch (o) {
#define FE_SPEC_LAUNCH(L)                                                                      \
        case L:                                                                                 \
            hipLaunchKernelGGL((fe_spectrum_kernel<L, int16_t>),                                \
                               dim3((G.n_grp_frames + fe_spec_waves(L) - 1) / fe_spec_waves(L)), \
                               dim3(64 * fe_spec_waves(L)), 0, st, G);                          \
            break;
        FE_SPEC_LAUNCH(6)
        FE_SPEC_LAUNCH(7)
        FE_SPEC_LAUNCH(8)
        FE_SPEC_LAUNCH(9)
        FE_SPEC_LAUNCH(10)
        FE_SPEC_LAUNCH(11)
        FE_SPEC_LAUNCH(12)
        FE_SPEC_LAUNCH(13)
#undef FE_SPEC_LAUNCH
        }
        /* (after the table above: the order of first launch places the template kernels in the
         * code object, DESIGN 6a) */
        else if (any == nullptr) switch (o) {
#define FE_SPEC_F32_LAUNCH(L)                                                                   \
        case L:                                                                                 \
            hipLaunchKernelGGL((fe_spectrum_kernel<L, float>),                                  \
                               dim3((G.n_grp_frames + fe_spec_waves(L) - 1) / fe_spec_waves(L)), \
                               dim3(64 * fe_spec_waves(L)), 0, st, G);                          \
            break;
        FE_SPEC_F32_LAUNCH(6)
        FE_SPEC_F32_LAUNCH(7)
        FE_SPEC_F32_LAUNCH(8)
        FE_SPEC_F32_LAUNCH(9)
        FE_SPEC_F32_LAUNCH(10)
        FE_SPEC_F32_LAUNCH(11)
        FE_SPEC_F32_LAUNCH(12)
        FE_SPEC_F32_LAUNCH(13)
#undef FE_SPEC_F32_LAUNCH
        }
        else {
            FeAnyParams A;
            A.P = G;
            A.any = m->d_fe_any_tab;
            A.dc = grp_dc[o];
#define FE_SPEC_ANY_LAUNCH(L, S)                                                                \
            case L:                                                                             \
                hipLaunchKernelGGL((fe_spectrum_any_kernel<L, S>),                              \
                                   dim3((G.n_grp_frames + fe_spec_waves(L) - 1) / fe_spec_waves(L)), \
                                   dim3(64 * fe_spec_waves(L)), 0, st, A);                      \
                break;
#define FE_SPEC_ANY_SWITCH(S)                                                                   \
            switch (o) {                                                                        \
                FE_SPEC_ANY_LAUNCH(6, S)                                                        \
                FE_SPEC_ANY_LAUNCH(7, S)                                                        \
                FE_SPEC_ANY_LAUNCH(8, S)                                                        \
                FE_SPEC_ANY_LAUNCH(9, S)                                                        \
                FE_SPEC_ANY_LAUNCH(10, S)                                                       \
                FE_SPEC_ANY_LAUNCH(11, S)                                                       \
                FE_SPEC_ANY_LAUNCH(12, S)                                                       \
                FE_SPEC_ANY_LAUNCH(13, S)                                                       \
            }
            if (!f32)
                FE_SPEC_ANY_SWITCH(int16_t)
            else
                FE_SPEC_ANY_SWITCH(float)
#undef FE_SPEC_ANY_SWITCH
#undef FE_SPEC_ANY_LAUNCH
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[1], st);
    if (e == hipSuccess && noise) {
        hipLaunchKernelGGL(fe_noise_kernel, dim3(n_utts), dim3(64), 0, st, F);
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[2], st);
    if (e == hipSuccess && any == nullptr) {
        hipLaunchKernelGGL(fe_cep_kernel, dim3((n_frames + FE_CEP_FRAMES - 1) / FE_CEP_FRAMES),
                           dim3(FE_CEP_THREADS), 0, st, F);
        e = hipGetLastError();
    } else if (e == hipSuccess) {
        FeAnyParams A;
        A.P = F;
        A.any = m->d_fe_any_tab;
        A.dc = SSW_FE_DC_NONE;
        hipLaunchKernelGGL(fe_cep_any_kernel,
                           dim3((n_frames + FE_CEP_FRAMES - 1) / FE_CEP_FRAMES),
                           dim3(FE_CEP_THREADS), 0, st, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[3], st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ssw_set_error("%s: %s", who, hipGetErrorString(e));
        return -1;
    }
    m->fe_timed = timed;
    return 0;
}

extern "C" int
ssw_fe_batch(ssw_model_t *m, const ssw_fe_config_t *cfg, const int16_t *d_pcm,
             const int64_t *samp_off, int32_t n_utts, float *d_cep, int32_t *frame_off_out,
             void *stream)
{
    return fe_batch(m, cfg, d_pcm, samp_off, NULL, n_utts, d_cep, frame_off_out, stream, false,
                    false, "ssw_fe_batch");
}

extern "C" int
ssw_fe_batch_ex(ssw_model_t *m, const ssw_fe_config_t *cfg, const int16_t *d_pcm,
                const int64_t *samp_off, const double *samprate, int32_t n_utts, float *d_cep,
                int32_t *frame_off_out, void *stream)
{
    return fe_batch(m, cfg, d_pcm, samp_off, samprate, n_utts, d_cep, frame_off_out, stream, true,
                    false, "ssw_fe_batch_ex");
}

extern "C" int
ssw_fe_batch_f32(ssw_model_t *m, const ssw_fe_config_t *cfg, const float *d_pcm,
                 const int64_t *samp_off, const double *samprate, int32_t n_utts, float *d_cep,
                 int32_t *frame_off_out, void *stream)
{
    return fe_batch(m, cfg, d_pcm, samp_off, samprate, n_utts, d_cep, frame_off_out, stream, true,
                    true, "ssw_fe_batch_f32");
}

extern "C" int
ssw_fe_kernel_timing(ssw_model_t *m, float ms[3])
{
    if (m == NULL || ms == NULL || !m->fe_timed) {
        ssw_set_error("no timed ssw_fe_batch or ssw_fe_batch_ex call (ssw_set_kernel_timing first)");
        return -1;
    }
    for (int k = 0; k < 3; ++k)
        HIP_OK(hipEventElapsedTime(&ms[k], m->fe_ev[k], m->fe_ev[k + 1]));
    return 0;
}
