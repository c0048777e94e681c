/* ssw_host_fe_any.inc -- host: ssw_fe_create, ssw_fe_batch_any and what goes with them.
 * Part of the single translation unit ssw_kernels.hip (included there, after ssw_host_fe.inc). */
/* ---------------------------------------------------------------------------------- */
/* The front end in every configuration fe_init accepts                                  */
/* ---------------------------------------------------------------------------------- */
static const char *
fe_host_endian()
{
    const uint16_t one = 1;
    return *(const unsigned char *)&one ? "little" : "big";
}

extern "C" ssw_fe_t *
ssw_fe_create(ssw_model_t *m, const ssw_fe_config_t *cfg, const char *warp_type,
              const char *warp_params)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to ssw_fe_create");
        return NULL;
    }
    const ssw_host_model_t *h = m->h;
    if (cfg == NULL) { /* the model's own settings, with the strings it read beside them */
        if (h->fe_err[0]) {
            ssw_set_error("ssw_fe_create: the model's feat_params.json cannot be used: %s",
                          h->fe_err);
            return NULL;
        }
        const char *host_endian = fe_host_endian();
        if (strcmp(h->fe_str.input_endian, host_endian) != 0) {
            ssw_set_error("ssw_fe_create: input_endian %s is not the host's (%s): byte-swapped "
                          "input is not supported", h->fe_str.input_endian, host_endian);
            return NULL;
        }
        cfg = &h->fe;
        if (warp_type == NULL)
            warp_type = h->fe_str.warp_type;
        if (warp_params == NULL)
            warp_params = h->fe_str.warp_params;
    }
    std::unique_ptr<ssw_fe_s> fe(new ssw_fe_s());
    if (ssw_fe_resolve(cfg, warp_type, warp_params, fe.get()) < 0)
        return NULL;
    fe->cfg.from_file = 0;
    return fe.release();
}

extern "C" void
ssw_fe_free(ssw_fe_t *fe)
{
    delete fe;
}

extern "C" int32_t
ssw_fe_out_dim(const ssw_fe_t *fe)
{
    if (fe == NULL) {
        ssw_set_error("bad arguments to ssw_fe_out_dim");
        return -1;
    }
    return fe->out_dim;
}

extern "C" int64_t
ssw_fe_frames(const ssw_fe_t *fe, double samprate, int64_t n_samples)
{
    if (fe == NULL || n_samples < 0) {
        ssw_set_error("bad arguments to ssw_fe_frames");
        return -1;
    }
    ssw_fe_framing_t f;
    if (ssw_fe_framing(&fe->cfg, samprate, &f) < 0)
        return -1;
    return ssw_fe_frames_at(&f, n_samples);
}

extern "C" int
ssw_fe_batch_any(ssw_model_t *m, ssw_fe_t *fe, const void *d_pcm, int32_t sample_type,
                 const int64_t *samp_off, const double *samprate, int32_t n_utts, float *d_cep,
                 int32_t *frame_off_out, void *stream)
{
    if (fe == NULL || (sample_type != 0 && sample_type != 1)) {
        ssw_set_error("bad arguments to ssw_fe_batch_any");
        return -1;
    }
    /* a configuration the existing entry points take runs their kernels: their bytes */
    return fe_batch(m, &fe->cfg, d_pcm, samp_off, samprate, n_utts, d_cep, frame_off_out, stream,
                    true, sample_type == 1, "ssw_fe_batch_any", fe->plain ? nullptr : fe);
}

extern "C" int
ssw_model_fe_plain(const ssw_model_t *m)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to ssw_model_fe_plain");
        return -1;
    }
    if (m->h->fe_err[0]) /* (they say why the file cannot be used) */
        return 1;
    return m->h->fe_str.warp_params[0] == '\0'
        && strcmp(m->h->fe_str.input_endian, fe_host_endian()) == 0
        && ssw_fe_config_check_ex(&m->h->fe) == 0;
}

extern "C" int
ssw_model_fe_warp(const ssw_model_t *m, char *type, int32_t type_len, char *params,
                  int32_t params_len)
{
    if (m == NULL || type == NULL || params == NULL || type_len < 1 || params_len < 1) {
        ssw_set_error("bad arguments to ssw_model_fe_warp");
        return -1;
    }
    snprintf(type, (size_t)type_len, "%s", m->h->fe_str.warp_type);
    snprintf(params, (size_t)params_len, "%s", m->h->fe_str.warp_params);
    return 0;
}
