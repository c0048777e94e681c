/* ssw_host_featex.inc -- host: ssw_feat_create and its accessors, ssw_feat_batch_ex,
 * ssw_model_feat_config.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order: last). */
/* ---------------------------------------------------------------------------------- */
/* dynamic features as the model says (feat types, CMN modes, varnorm, LDA, svspec)     */
/* ---------------------------------------------------------------------------------- */
struct ssw_feat_s {
    ssw_model_s *m;
    ssw_feat_plan_t plan;
    unsigned char *d_tab; /* recipe | lda_t | sv, each at a 256-byte boundary */
    size_t off_lda, off_sv;
    int tf;               /* frames per tile */
    size_t lds;           /* bytes of LDS a tile takes */
};

constexpr size_t FEATEX_LDS_BUDGET = 64 * 1024;

extern "C" int
ssw_model_feat_config(const ssw_model_t *m, ssw_feat_config_t *out)
{
    if (m == NULL || out == NULL) {
        ssw_set_error("bad arguments to ssw_model_feat_config");
        return -1;
    }
    *out = m->h->feat;
    return 0;
}

extern "C" void
ssw_feat_free(ssw_feat_t *f)
{
    if (f == NULL)
        return;
    if (f->d_tab != NULL)
        (void)hipFree(f->d_tab);
    ssw_feat_plan_free(&f->plan);
    delete f;
}

extern "C" ssw_feat_t *
ssw_feat_create(ssw_model_t *m, const ssw_feat_config_t *cfg)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to ssw_feat_create");
        return NULL;
    }
    if (cfg == NULL && m->h->feat_err[0]) {
        ssw_set_error("ssw_feat_create: the model's feat_params.json cannot be used: %s",
                      m->h->feat_err);
        return NULL;
    }
    std::unique_ptr<ssw_feat_s> f(new ssw_feat_s());
    f->m = m;
    f->d_tab = NULL;
    /* every refusal comes from here, before anything is uploaded */
    if (ssw_feat_plan_build(cfg != NULL ? cfg : &m->h->feat, &f->plan) < 0)
        return NULL;
    const ssw_feat_plan_t &p = f->plan;
    f->tf = feat_tile_frames(p.cepsize, p.window, p.raw_dim, p.lda_rows, p.sv != NULL,
                             FEATEX_LDS_BUDGET, &f->lds);
    if (f->tf < 1) {
        ssw_set_error("ssw_feat_create: one frame of %d raw dimensions with a window of %d does not "
                      "fit %zu bytes of LDS", p.raw_dim, p.window, FEATEX_LDS_BUDGET);
        ssw_feat_plan_free(&f->plan);
        return NULL;
    }
    if (m->device != SSW_DEVICE_NONE) {
        WsLayout L;
        L.in(p.recipe, sizeof(uint32_t) * (size_t)p.raw_dim);
        f->off_lda = L.in(p.lda_t, sizeof(float) * (size_t)p.raw_dim * (size_t)p.lda_rows);
        f->off_sv = L.in(p.sv, sizeof(int32_t) * (size_t)p.sv_dim);
        std::vector<unsigned char> stage(L.in_bytes());
        L.fill(stage.data(), 0);
        if (hipSetDevice(m->device) != hipSuccess
            || hipMalloc((void **)&f->d_tab, L.size()) != hipSuccess
            || hipMemcpy(f->d_tab, stage.data(), stage.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            ssw_set_error("ssw_feat_create: cannot upload %zu bytes of tables", L.size());
            if (f->d_tab != NULL)
                (void)hipFree(f->d_tab);
            ssw_feat_plan_free(&f->plan);
            return NULL;
        }
    }
    return f.release();
}

extern "C" int32_t
ssw_feat_out_dim(const ssw_feat_t *f)
{
    return f != NULL ? f->plan.out_dim : -1;
}

extern "C" int32_t
ssw_feat_raw_dim(const ssw_feat_t *f)
{
    return f != NULL ? f->plan.raw_dim : -1;
}

extern "C" int32_t
ssw_feat_window(const ssw_feat_t *f)
{
    return f != NULL ? f->plan.window : -1;
}

extern "C" int32_t
ssw_feat_n_streams(const ssw_feat_t *f)
{
    return f == NULL ? -1 : f->plan.n_sv ? f->plan.n_sv : f->plan.n_stream;
}

extern "C" int32_t
ssw_feat_stream_len(const ssw_feat_t *f, int32_t i)
{
    if (f == NULL || i < 0 || i >= ssw_feat_n_streams(f))
        return -1;
    const ssw_feat_plan_t &p = f->plan; /* feat_dimension2, include/soundswallower/feat.h:148 */
    return p.lda_rows ? p.lda_rows : p.n_sv ? p.sv_len[i] : p.stream_len[i];
}

extern "C" int32_t
ssw_feat_tile_frames(const ssw_feat_t *f)
{
    return f != NULL ? f->tf : -1;
}

extern "C" int
ssw_feat_cmn_prior(const ssw_feat_t *f, ssw_cmn_state_t *out)
{
    if (f == NULL || out == NULL) {
        ssw_set_error("bad arguments to ssw_feat_cmn_prior");
        return -1;
    }
    memset(out, 0, sizeof(*out));
    memcpy(out->mean, f->plan.prior_mean, sizeof(float) * (size_t)f->plan.cepsize);
    memcpy(out->sum, f->plan.prior_sum, sizeof(float) * (size_t)f->plan.cepsize);
    out->nframe = f->plan.prior_nframe;
    return 0;
}

extern "C" int
ssw_feat_batch_ex(ssw_model_t *m, ssw_feat_t *feat, const float *d_cep, int32_t n_frames,
                  const int32_t *utt_off, int32_t n_utts, int32_t ncep, float *d_out,
                  ssw_cmn_state_t *cmn_state, void *stream)
{
    if (m == NULL) {
        ssw_set_error("bad arguments to ssw_feat_batch_ex");
        return -1;
    }
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    if (feat == NULL) {
        if (m->own_feat == NULL && (m->own_feat = ssw_feat_create(m, NULL)) == NULL)
            return -1;
        feat = m->own_feat;
    }
    if (feat->m != m) {
        ssw_set_error("ssw_feat_batch_ex: the configuration was created for another model");
        return -1;
    }
    const ssw_feat_plan_t &p = feat->plan;
    const int C = p.cepsize;
    if (ncep != C) {
        ssw_set_error("ssw_feat_batch_ex: %d cepstra per frame, but the configuration's ceplen is %d",
                      ncep, C);
        return -1;
    }
    std::vector<int32_t> tiles;
    const long n_tiles = feat_tiles_build(utt_off, n_utts, n_frames, feat->tf, tiles);
    if (n_tiles < 0) {
        ssw_set_error("bad arguments to ssw_feat_batch_ex (utt_off must run from 0 to n_frames "
                      "without decreasing)");
        return -1;
    }
    const bool chain = p.cmn == SSW_CMN_LIVE && cmn_state != NULL;
    if (n_utts == 0 || (n_frames == 0 && !chain))
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (n_frames > 0 && (d_cep == NULL || d_out == NULL)) {
        ssw_set_error("bad arguments to ssw_feat_batch_ex");
        return -1;
    }
    if (chain && (cmn_state->nframe < 0 || cmn_state->nframe > (1 << 30))) {
        ssw_set_error("ssw_feat_batch_ex: cmn_state holds %d frames", cmn_state->nframe);
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    /* the workspace: what is uploaded (tiles, offsets, the state going in), then the state
     * coming out, the means and the scales */
    float h_state[2 * SSW_FEAT_MAX_CEP + 1];
    {
        const float *mean = chain ? cmn_state->mean : p.prior_mean;
        const float *sum = chain ? cmn_state->sum : p.prior_sum;
        const int32_t nframe = chain ? cmn_state->nframe : p.prior_nframe;
        memcpy(h_state, mean, sizeof(float) * (size_t)C);
        memcpy(h_state + C, sum, sizeof(float) * (size_t)C);
        memcpy(h_state + 2 * C, &nframe, sizeof(int32_t));
    }
    const size_t state_bytes = sizeof(float) * (size_t)(2 * C + 1);
    WsLayout L;
    const size_t off_tiles = L.in(tiles.data(), sizeof(int32_t) * tiles.size());
    const size_t off_utt = L.in(utt_off, sizeof(int32_t) * ((size_t)n_utts + 1));
    const size_t off_state = L.in(h_state, state_bytes, 2 * state_bytes);
    const size_t off_mean = L.out(sizeof(float) * (size_t)n_utts * C);
    const size_t off_scale = L.out(sizeof(float) * (size_t)n_utts * C);
    if (devbuf_reserve(m->featex_ws, L.size(), "ssw_feat_batch_ex") < 0)
        return -1;
    unsigned char *ws = m->featex_ws.p;
    if (stage_upload(m, ws, L.in_bytes(), st, [&](unsigned char *hs) { L.fill(hs, 0); }) < 0)
        return -1;
    FeatExParams P;
    P.cep = d_cep;
    P.utt_off = ws_at<const int>(ws, off_utt);
    P.tiles = ws_at<const FeatTile>(ws, off_tiles);
    P.recipe = ws_at<const uint32_t>(feat->d_tab, 0);
    P.lda_t = p.lda_rows ? ws_at<const float>(feat->d_tab, feat->off_lda) : nullptr;
    P.sv = p.sv != NULL ? ws_at<const int>(feat->d_tab, feat->off_sv) : nullptr;
    P.mean = ws_at<float>(ws, off_mean);
    P.scale = ws_at<float>(ws, off_scale);
    P.state = ws_at<float>(ws, off_state);
    P.out = d_out;
    P.n_utts = n_utts;
    P.C = C;
    P.window = p.window;
    P.raw_dim = p.raw_dim;
    P.lda_rows = p.lda_rows;
    P.sv_dim = p.sv_dim;
    P.out_dim = p.out_dim;
    P.tf = feat->tf;
    P.cmn = p.cmn;
    P.varnorm = p.varnorm;
    hipError_t e = hipSuccess;
    if (chain) {
        hipLaunchKernelGGL(feat_chain_kernel, dim3(1), dim3(FEATEX_THREADS), 0, st, P);
        e = hipGetLastError();
    } else if (p.cmn != SSW_CMN_NONE) {
        hipLaunchKernelGGL(feat_stats_kernel, dim3(n_utts), dim3(FEATEX_THREADS), 0, st, P);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_tiles > 0) {
        hipLaunchKernelGGL(feat_tile_kernel, dim3((unsigned)n_tiles), dim3(FEATEX_THREADS), feat->lds,
                           st, P);
        e = hipGetLastError();
    }
    float h_after[2 * SSW_FEAT_MAX_CEP + 1];
    if (e == hipSuccess && chain)
        e = hipMemcpyAsync(h_after, ws + off_state + state_bytes, state_bytes, hipMemcpyDeviceToHost,
                           st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ssw_set_error("ssw_feat_batch_ex: %s", hipGetErrorString(e));
        return -1;
    }
    if (chain) {
        memcpy(cmn_state->mean, h_after, sizeof(float) * (size_t)C);
        memcpy(cmn_state->sum, h_after + C, sizeof(float) * (size_t)C);
        memcpy(&cmn_state->nframe, h_after + 2 * C, sizeof(int32_t));
    }
    return 0;
}
