/* ssw_host_cont_listed.inc -- host: a continuous-density model in the reference's default
 * configuration (compallsen = no): the launches of cont_listed_kernel (ssw_k11_cont.inc), the
 * second pass over bitmap rows, and the kernel's test surface.  ssw_model_enable_active
 * (ssw_host_model.inc) makes the table these read.
 * Part of the single translation unit ssw_kernels.hip, included LAST: the kernel is emitted behind
 * every other one, whose placement in the code object stays as it was. */

/* the kernel's dynamic LDS for lists of up to `cap` senones (fpa_shape checks the same carve
 * against a CU's) */
static size_t
cont_listed_lds(const ssw_model_s *m, int cap)
{
    return ContListedCarve(m->h->veclen_total, cap).bytes();
}

static int
cont_listed_launch(ssw_model_s *m, const ContListedReq &Q, hipStream_t st)
{
    const ssw_host_model_t *h = m->h;
    if (m->d_cont_rec_sm == NULL) {
        ssw_set_error("internal error: the listed-senone kernel without its table");
        return -1;
    }
    if (Q.n_frames <= 0)
        return 0;
    ContListedParams P;
    memset(&P, 0, sizeof(P));
    P.tab = m->d_cont_rec_sm;
    P.pdf = m->d_cont_pdf;
    P.logadd8 = m->d_logadd8;
    P.feats = Q.d_feats;
    P.listed = Q.d_listed;
    P.row_of_frame = Q.d_row_of_frame;
    P.out = Q.d_out;
    P.yes = Q.d_yes;
    P.n_frames = Q.n_frames;
    P.n_sen = h->n_sen;
    P.nw32 = (h->n_sen + 31) / 32;
    P.n_feat = h->n_feat;
    P.n_density = h->n_density;
    P.featdim = h->veclen_total;
    P.aw = h->cfg.aw;
    P.zero = h->zero8;
    P.topn = h->cfg.topn >= h->n_density || h->cfg.topn < 1 ? 0 : h->cfg.topn;
    P.cap = Q.cap <= 0 || Q.cap > h->n_sen ? h->n_sen : Q.cap;
    P.full = Q.full;
    for (int f = 0; f < h->n_feat; ++f) {
        P.featoff[f] = h->featoff[f];
        P.veclen[f] = h->veclen[f];
        P.rec_off[f] = (unsigned long long)h->cont_sm_off[f];
    }
    P.sen_floats = (unsigned long long)h->cont_sm_sen;
    if (P.topn > SSW_CONT_MAX_TOPN) { /* (the loader's refusal, build_cont_records) */
        ssw_set_error("continuous model: topn %d, at most %d or all densities", P.topn, SSW_CONT_MAX_TOPN);
        return -1;
    }
    const size_t lds = cont_listed_lds(m, P.cap);
    if (lds > 156 * 1024) {
        ssw_set_error("continuous model: lists of up to %d senones need %zu KB of LDS per workgroup "
                      "(160 KB a CU)", P.cap, lds / 1024);
        return -1;
    }
    int log2g = 0;
    while ((1 << log2g) < h->n_density)
        ++log2g;
    const dim3 grid((unsigned)((Q.n_frames + 3) / 4));
#define SSW_CONT_LISTED(N)                                                                         \
    case N:                                                                                        \
        if (lds > 48 * 1024)                                                                       \
            HIP_OK(hipFuncSetAttribute((const void *)cont_listed_kernel<N>,                        \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));     \
        hipLaunchKernelGGL(cont_listed_kernel<N>, grid, dim3(256), lds, st, P);                    \
        break
    switch (log2g) {
        SSW_CONT_LISTED(0);
        SSW_CONT_LISTED(1);
        SSW_CONT_LISTED(2);
        SSW_CONT_LISTED(3);
        SSW_CONT_LISTED(4);
        SSW_CONT_LISTED(5);
        SSW_CONT_LISTED(6);
    default:
        ssw_set_error("continuous model: %d densities, at most %d are supported", h->n_density,
                      SSW_CONT_MAX_DENSITY);
        return -1;
    }
#undef SSW_CONT_LISTED
    HIP_OK(hipGetLastError());
    if (m->sw.timing) { /* (one kernel: no split) */
        HIP_OK(hipEventRecord(m->sw.ev[1], st));
        HIP_OK(hipEventRecord(m->sw.ev[2], st));
        m->sw.timing_pieced = 0;
    }
    return 0;
}

/* ssw_align_batch_active_ex on a continuous model (align_batch_active_impl has checked the
 * arguments and set the device): ActiveSetBuilder's set of every segment as one bitmap row
 * (cont_active_rows), a row_of_frame table, the rows scored full-width into the model's text-row
 * workspace (or d_senscr), and the alignment over full rows. */
static int
cont_align_active(ssw_model_t *m, const float *d_feats, int32_t n_utts, const int32_t *frame_off,
                  const int32_t *phone_off, const uint16_t *senid, const int16_t *tmatid,
                  const int32_t *sf, const int32_t *ef, const uint32_t *seed_active,
                  ssw_align_entry_t *state_io, int32_t *status, int16_t *d_senscr, void *stream)
{
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    const int n_frames = frame_off[n_utts];
    const size_t nw32 = ((size_t)h->n_sen + 31) / 32;
    std::vector<uint32_t> rows;
    std::vector<int32_t> row_of_frame((size_t)std::max(n_frames, 1), 0);
    for (int u = 0; u < n_utts; ++u) {
        const int f0 = frame_off[u], p0 = phone_off[u];
        if (cont_active_rows(h->n_sen, frame_off[u + 1] - f0, phone_off[u + 1] - p0,
                             senid + (size_t)p0 * 3, sf + p0, ef + p0,
                             seed_active != NULL ? seed_active + (size_t)u * nw32 : NULL,
                             (int32_t)(rows.size() / nw32), rows, row_of_frame.data() + f0) < 0)
            return -1;
    }
    int16_t *d_rows = d_senscr;
    if (d_rows == NULL) {
        if (text_rows_reserve(m, n_frames, "ssw_align_batch_active") < 0)
            return -1;
        d_rows = m->text_scr.as<int16_t>();
    }
    if (n_frames > 0) {
        WsLayout L;
        const size_t o_rof = L.out(sizeof(int32_t) * (size_t)n_frames);
        const size_t o_rows = L.out(sizeof(uint32_t) * std::max(rows.size(), (size_t)1));
        if (devbuf_reserve(m->cont_act_ws, L.size(), "ssw_align_batch_active") < 0)
            return -1;
        unsigned char *ws = m->cont_act_ws.p;
        HIP_OK(hipMemcpyAsync(ws + o_rof, row_of_frame.data(), sizeof(int32_t) * (size_t)n_frames,
                              hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(ws + o_rows, rows.data(), sizeof(uint32_t) * rows.size(),
                              hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st)); /* the host vectors go out of scope before the kernels end */
        SenoneListedParams Ls;
        memset(&Ls, 0, sizeof(Ls));
        Ls.listed = ws_at<uint32_t>(ws, o_rows);
        Ls.out = d_rows;
        Ls.full = 1;
        Ls.cap = h->n_sen;
        ActiveSets act;
        act.seg_of_frame = NULL;
        act.seg_cbmask = NULL;
        act.a2 = NULL;
        act.ls = &Ls;
        act.row_of_frame = ws_at<int32_t>(ws, o_rof);
        ScoreReq R{};
        R.scorer = SSW_SCORER_MS;
        R.d_feats = d_feats;
        R.n_frames = n_frames;
        R.utt_off = frame_off;
        R.n_utts = n_utts;
        R.d_out = d_rows;
        R.stream = stream;
        R.act = &act;
        if (score_batch_impl(m, R) < 0)
            return -1;
    }
    return align_batch_levels(m, d_rows, n_utts, frame_off, phone_off, senid, tmatid, sf, ef, state_io,
                              status, stream, NULL);
}

extern "C" int
ssw_debug_cont_score_listed(ssw_model_t *m, const float *d_feats, int32_t n_frames,
                            const uint32_t *listed, int32_t full, int16_t *d_out, void *stream)
{
    if (m == NULL || n_frames < 0 || (n_frames > 0 && (!d_feats || !listed || !d_out))
        || (full != 0 && full != 1)) {
        ssw_set_error("bad arguments to ssw_debug_cont_score_listed");
        return -1;
    }
    if (check_has_device(m) < 0)
        return -1;
    if (!m->h->continuous) {
        ssw_set_error("ssw_debug_cont_score_listed: the model is not continuous (one codebook per "
                      "senone)");
        return -1;
    }
    if (cont_refuse_active(m, "ssw_debug_cont_score_listed") < 0
        || cont_check_shape(m, SSW_SCORER_MS) < 0)
        return -1;
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    if (n_frames == 0)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipSetDevice(m->device));
    const size_t bytes = sizeof(uint32_t) * (size_t)n_frames * (((size_t)m->h->n_sen + 31) / 32);
    if (devbuf_reserve(m->cont_act_ws, bytes, "ssw_debug_cont_score_listed") < 0)
        return -1;
    HIP_OK(hipMemcpyAsync(m->cont_act_ws.p, listed, bytes, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); /* (the caller's array is free again on return) */
    ContListedReq Q{ d_feats, n_frames, m->cont_act_ws.as<uint32_t>(), NULL, d_out, NULL, 0, full };
    return cont_listed_launch(m, Q, st);
}
