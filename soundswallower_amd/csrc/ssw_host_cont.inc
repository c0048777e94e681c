/* ssw_host_cont.inc -- host: the ms scorer's launches on a continuous-density model
 * (ssw_k11_cont.inc).  Part of the single translation unit ssw_kernels.hip (included there, in
 * this order). */

/* what the entry points that take a scorer refuse of a continuous model; -1 with the message set */
static int
cont_check_shape(const ssw_model_s *m, int scorer)
{
    const ssw_host_model_t *h = m->h;
    if (scorer != SSW_SCORER_MS) {
        ssw_set_error("a continuous model (one codebook per senone) is scored with SSW_SCORER_MS "
                      "(scorer %d asked)", scorer);
        return -1;
    }
    if (getenv("SSW_SCAN") != NULL || m->kn.scan_audit > 0) {
        ssw_set_error("SSW_SCAN / SSW_SCAN_AUDIT: not available with a continuous model (one "
                      "codebook per senone): it has no top-N scan");
        return -1;
    }
    if (h->ms_pdf == NULL) {
        ssw_set_error("the ms scorer needs a mixture_weights file (src/ms_mgau.c:208-212)");
        return -1;
    }
    if (h->logadd8_size != 256 || h->cfg.aw == 0) {
        ssw_set_error("ms scorer: unsupported log base (add table of %d entries) or aw = 0",
                      h->logadd8_size);
        return -1;
    }
    return 0;
}

/* the calls that are out of scope for every continuous model (compact score rows, the views of
 * the PTM scan); -1 with the message set when `m` is one */
static int
cont_refuse(const ssw_model_s *m, const char *who)
{
    if (m == NULL || m->h == NULL || !m->h->continuous)
        return 0;
    ssw_set_error("%s: not available with a continuous model (one codebook per senone): it is "
                  "scored in whole rows only", who);
    return -1;
}

/* the *_active entry points: a continuous model is taken once ssw_model_enable_active has given
 * it the listed-senone kernel's table (ssw_host_cont_listed.inc); until then refused as above */
static int
cont_refuse_active(const ssw_model_s *m, const char *who)
{
    if (m == NULL || m->h == NULL || !m->h->continuous || m->d_cont_rec_sm != NULL)
        return 0;
    ssw_set_error("%s: not available with a continuous model (one codebook per senone): it is "
                  "scored in whole rows only (until ssw_model_enable_active is called on it)", who);
    return -1;
}

/* every (frame, senone) of one batch on `st`. The workspace takes 2 n_sen + 4 bytes per frame. */
static int
cont_launch(ssw_model_s *m, const float *d_feats, int32_t n_frames, int16_t *d_out, hipStream_t st)
{
    const ssw_host_model_t *h = m->h;
    const long long tiles = ((long long)n_frames + CONT_FR - 1) / CONT_FR;
    const int sen_blocks = (h->n_sen + CONT_THREADS - 1) / CONT_THREADS;
    if (tiles > 0x7fffffffll || sen_blocks > 65535) {
        ssw_set_error("continuous model: a batch of %d frames is too large for one launch", n_frames);
        return -1;
    }
    WsLayout L;
    const size_t o_min = L.out((size_t)n_frames * sizeof(int));
    const size_t o_raw = L.out((size_t)n_frames * (size_t)h->n_sen * sizeof(int16_t));
    if (devbuf_reserve(m->cont_ws, L.size(), "continuous-model scoring") < 0)
        return -1;
    ContParams P;
    memset(&P, 0, sizeof(P));
    P.fmin = ws_at<int>(m->cont_ws.p, o_min);
    P.raw = ws_at<int16_t>(m->cont_ws.p, o_raw);
    P.out = d_out;
    P.n_frames = n_frames;
    P.n_sen = h->n_sen;
    P.n_sp = h->cont_sp;
    P.n_feat = h->n_feat;
    P.n_density = h->n_density;
    P.featdim = h->veclen_total;
    P.aw = h->cfg.aw;
    P.zero = h->zero8;
    for (int f = 0; f < h->n_feat; ++f) {
        P.featoff[f] = h->featoff[f];
        P.veclen[f] = h->veclen[f];
        P.toff[f] = (unsigned long long)h->cont_off[f];
    }
    /* every byte 0x7f: above any int16 score */
    HIP_OK(hipMemsetAsync(P.fmin, 0x7f, (size_t)n_frames * sizeof(int), st));
    const dim3 grid((unsigned)tiles, (unsigned)sen_blocks);
    const int topn = h->cfg.topn >= h->n_density ? 0 : h->cfg.topn;
#define SSW_CONT_LAUNCH(N)                                                                   \
    case N:                                                                                  \
        hipLaunchKernelGGL(cont_score_kernel<N>, grid, dim3(CONT_THREADS), 0, st, m->d_cont_rec, \
                           m->d_cont_pdf, m->d_logadd8, d_feats, P);                         \
        break
    switch (topn) {
        SSW_CONT_LAUNCH(0);
        SSW_CONT_LAUNCH(1);
        SSW_CONT_LAUNCH(2);
        SSW_CONT_LAUNCH(3);
        SSW_CONT_LAUNCH(4);
        SSW_CONT_LAUNCH(5);
        SSW_CONT_LAUNCH(6);
        SSW_CONT_LAUNCH(7);
        SSW_CONT_LAUNCH(8);
    default:
        ssw_set_error("continuous model: topn %d, at most %d or all densities", topn,
                      SSW_CONT_MAX_TOPN);
        return -1;
    }
#undef SSW_CONT_LAUNCH
    HIP_OK(hipGetLastError());
    if (m->sw.timing)
        HIP_OK(hipEventRecord(m->sw.ev[1], st));
    if (m->ms_raw)
        hipLaunchKernelGGL(cont_norm_kernel<true>, dim3((unsigned)n_frames), dim3(256), 0, st, P);
    else
        hipLaunchKernelGGL(cont_norm_kernel<false>, dim3((unsigned)n_frames), dim3(256), 0, st, P);
    HIP_OK(hipGetLastError());
    if (m->sw.timing) {
        HIP_OK(hipEventRecord(m->sw.ev[2], st));
        m->sw.timing_pieced = 0;
    }
    return 0;
}
