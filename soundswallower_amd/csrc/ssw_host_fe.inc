/* ssw_host_fe.inc -- host: ssw_fe_batch, ssw_fe_frame_count, ssw_model_fe_config.
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

/* the tables for configuration c on the host when the device copy was built for another one
 * (NULL and *ok when it is current; building them is also the last check of c) */
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

extern "C" int
ssw_fe_batch(ssw_model_t *m, const ssw_fe_config_t *cfg, const int16_t *d_pcm,
             const int64_t *samp_off, int32_t n_utts, float *d_cep, int32_t *frame_off_out,
             void *stream)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to ssw_fe_batch");
        return -1;
    }
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    if (n_utts < 0 || samp_off == NULL || frame_off_out == NULL || samp_off[0] != 0) {
        ssw_set_error("bad arguments to ssw_fe_batch");
        return -1;
    }
    if (cfg == NULL && m->h->fe_err[0]) {
        ssw_set_error("ssw_fe_batch: the model's feat_params.json cannot be used: %s",
                      m->h->fe_err);
        return -1;
    }
    const ssw_fe_config_t *c = cfg != NULL ? cfg : &m->h->fe;
    ssw_fe_config_t key;
    bool ok;
    std::unique_ptr<ssw_fe_tables_t> fresh = fe_tables_if_new(m, c, &key, &ok);
    if (!ok)
        return -1;
    int64_t total = 0;
    frame_off_out[0] = 0;
    for (int32_t u = 0; u < n_utts; ++u) {
        const int64_t n = samp_off[u + 1] - samp_off[u];
        if (n < 0) {
            ssw_set_error("ssw_fe_batch: samp_off decreases at utterance %d", u);
            return -1;
        }
        total += ssw_fe_frames_of(n);
        if (total > INT32_MAX) {
            ssw_set_error("ssw_fe_batch: more than 2^31 - 1 frames in one batch");
            return -1;
        }
        frame_off_out[u + 1] = (int32_t)total;
    }
    if (total == 0)
        return 0;
    if (m->device == SSW_DEVICE_NONE) {
        ssw_set_error("model was loaded with device = SSW_DEVICE_NONE: no GPU, no CPU fallback");
        return -1;
    }
    if (d_pcm == NULL || d_cep == NULL) {
        ssw_set_error("bad arguments to ssw_fe_batch");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    if (fresh && fe_tables_upload(m, fresh.get(), &key) < 0)
        return -1;
    const int n_frames = (int)total, nfilt = m->fe_nfilt;
    /* grow-only workspace: offsets, then the mel spectra */
    const size_t off_bytes = (((size_t)n_utts + 1) * (sizeof(long long) + sizeof(int)) + 255) & ~(size_t)255;
    const size_t ws = off_bytes + (size_t)n_frames * nfilt * sizeof(double);
    if (ws > m->fe_ws_cap) {
        (void)hipFree(m->d_fe_ws);
        m->d_fe_ws = NULL;
        m->fe_ws_cap = 0;
        HIP_OK(hipMalloc((void **)&m->d_fe_ws, ws));
        m->fe_ws_cap = ws;
    }
    long long *d_soff = (long long *)m->d_fe_ws;
    int *d_foff = (int *)(d_soff + n_utts + 1);
    FeParams F;
    F.pcm = d_pcm;
    F.samp_off = d_soff;
    F.frame_off = d_foff;
    F.tab = m->d_fe_tab;
    F.mfspec = (double *)(m->d_fe_ws + off_bytes);
    F.cep = d_cep;
    F.n_utts = n_utts;
    F.n_frames = n_frames;
    if (m->timing && !m->fe_ev_ready) {
        for (int i = 0; i < 4; ++i)
            HIP_OK(hipEventCreate(&m->fe_ev[i]));
        m->fe_ev_ready = 1;
    }
    const bool timed = m->timing && m->fe_ev_ready;
    hipError_t e = hipMemcpyAsync(d_soff, samp_off, sizeof(long long) * ((size_t)n_utts + 1),
                                  hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_foff, frame_off_out, sizeof(int) * ((size_t)n_utts + 1),
                           hipMemcpyHostToDevice, st);
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[0], st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fe_spectrum_kernel, dim3((n_frames + FE_SPEC_WAVES - 1) / FE_SPEC_WAVES),
                           dim3(64 * FE_SPEC_WAVES), 0, st, F);
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[1], st);
    if (e == hipSuccess && m->fe_noise) {
        hipLaunchKernelGGL(fe_noise_kernel, dim3(n_utts), dim3(64), 0, st, F);
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[2], st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fe_cep_kernel, dim3((n_frames + FE_CEP_FRAMES - 1) / FE_CEP_FRAMES),
                           dim3(FE_CEP_THREADS), 0, st, F);
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed)
        e = hipEventRecord(m->fe_ev[3], st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ssw_set_error("ssw_fe_batch: %s", hipGetErrorString(e));
        return -1;
    }
    m->fe_timed = timed;
    return 0;
}

extern "C" int
ssw_fe_kernel_timing(ssw_model_t *m, float ms[3])
{
    if (m == NULL || ms == NULL || !m->fe_timed) {
        ssw_set_error("no timed ssw_fe_batch call (ssw_set_kernel_timing first)");
        return -1;
    }
    for (int k = 0; k < 3; ++k)
        HIP_OK(hipEventElapsedTime(&ms[k], m->fe_ev[k], m->fe_ev[k + 1]));
    return 0;
}
