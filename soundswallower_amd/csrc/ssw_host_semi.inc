/* ssw_host_semi.inc -- host: the s2_semi scorer's launches (ssw_k10_semi.inc).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */

/* what the entry points that take a scorer refuse for SSW_SCORER_S2_SEMI, and what they refuse of
 * a single-codebook model for the other two; -1 with the message set */
static int
semi_check_shape(const ssw_model_s *m, int scorer)
{
    const ssw_host_model_t *h = m->h;
    if (scorer != SSW_SCORER_S2_SEMI) {
        if (h->sc_rec == NULL)
            return 0;
        ssw_set_error("a single-codebook model is scored with SSW_SCORER_S2_SEMI (scorer %d asked)",
                      scorer);
        return -1;
    }
    if (h->sc_rec == NULL) {
        ssw_set_error("s2_semi scorer: the model has %d codebooks, not one (src/s2_semi_mgau.c:942)",
                      h->n_cb);
        return -1;
    }
    if (h->ptm_mixw == NULL) {
        ssw_set_error("s2_semi scorer: the model has no 8-bit mixture weights (sendump / mixw)");
        return -1;
    }
    if (h->logadd8_size != 256) { /* (as for PTM: the reference reads its whole table) */
        ssw_set_error("s2_semi scorer: unsupported log-add table (%d entries, the kernels hold 256)",
                      h->logadd8_size);
        return -1;
    }
    if (h->cfg.topn < 1 || h->cfg.topn > SSW_SC_MAX_TOPN) {
        ssw_set_error("s2_semi scorer: topn %d, 1 to %d are supported", h->cfg.topn, SSW_SC_MAX_TOPN);
        return -1;
    }
    return 0;
}

/* the calls that are out of scope for the s2_semi scorer (compact score rows, the alignment over
 * active sets); -1 with the message set when `scorer` is it */
static int
semi_refuse(int scorer, const char *who)
{
    if (scorer != SSW_SCORER_S2_SEMI)
        return 0;
    ssw_set_error("%s: not available with the s2_semi scorer (SSW_SCORER_S2_SEMI): it scores whole "
                  "rows only", who);
    return -1;
}

/* densities, chains and senones of one batch on `st`; C: the batch as fill_chain_params and
 * score_batch_impl describe it (offsets uploaded, carried rows in C.carry_pk).  The workspace
 * takes 1,569 bytes per (frame, stream). */
static int
semi_launch(ssw_model_s *m, const ChainParams &C, int16_t *d_out, hipStream_t st)
{
    const ssw_host_model_t *h = m->h;
    const size_t pairs = (size_t)C.n_frames * (size_t)h->n_feat;
    WsLayout L;
    const size_t o_row = L.out(pairs * SSW_SC_MAX_DENSITY * sizeof(int));
    const size_t o_tie = L.out(pairs * 4 * sizeof(unsigned long long));
    const size_t o_cand = L.out(pairs * 64 * sizeof(int2));
    const size_t o_hard = L.out(pairs);
    if (devbuf_reserve(m->sc_ws, L.size(), "s2_semi scoring") < 0)
        return -1;
    SemiParams P;
    memset(&P, 0, sizeof(P));
    P.rec = m->d_sc_rec;
    P.feats = C.feats;
    P.utt_off = C.utt_off;
    P.carry_pk = C.carry_pk;
    P.row_dint = ws_at<int>(m->sc_ws.p, o_row);
    P.row_tie = ws_at<unsigned long long>(m->sc_ws.p, o_tie);
    P.cand = ws_at<int2>(m->sc_ws.p, o_cand);
    P.hard = ws_at<uint8_t>(m->sc_ws.p, o_hard);
    P.topn_cw = C.topn_cw;
    P.topn_sc = C.topn_sc;
    P.mixw = m->d_sc_mixw;
    P.logadd8 = m->d_logadd8;
    P.out = d_out;
    P.n_utts = C.n_utts;
    P.n_frames = C.n_frames;
    P.n_feat = h->n_feat;
    P.n_density = h->n_density;
    P.featdim = h->veclen_total;
    P.ds = C.ds;
    P.frame_base = C.frame_base;
    P.chain_utts = C.chain_utts;
    P.topn = h->cfg.topn;
    P.n_sen = h->n_sen;
    P.sc_stride = m->sc_stride;
    for (int f = 0; f < h->n_feat; ++f) {
        P.featoff[f] = h->featoff[f];
        P.veclen[f] = h->veclen[f];
    }
    const long long waves = (long long)((C.n_frames + SEMI_FR - 1) / SEMI_FR) * h->n_feat;
    const long long sen_blocks = (long long)C.n_frames * ((h->n_sen + 1023) / 1024);
    if (waves / 4 + 1 > 0x7fffffffll || sen_blocks > 0x7fffffffll) {
        ssw_set_error("s2_semi scorer: a batch of %d frames is too large for one launch", C.n_frames);
        return -1;
    }
    hipLaunchKernelGGL(semi_density_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, P);
    HIP_OK(hipGetLastError());
    if (m->sw.timing)
        HIP_OK(hipEventRecord(m->sw.ev_sc, st));
    const dim3 chains((unsigned)((C.chain_utts ? 1 : C.n_utts) * h->n_feat));
    switch (P.topn) {
    case 1: hipLaunchKernelGGL(semi_chain_kernel<1>, chains, dim3(64), 0, st, P); break;
    case 2: hipLaunchKernelGGL(semi_chain_kernel<2>, chains, dim3(64), 0, st, P); break;
    case 3: hipLaunchKernelGGL(semi_chain_kernel<3>, chains, dim3(64), 0, st, P); break;
    default: hipLaunchKernelGGL(semi_chain_kernel<4>, chains, dim3(64), 0, st, P); break;
    }
    HIP_OK(hipGetLastError());
    if (m->sw.timing)
        HIP_OK(hipEventRecord(m->sw.ev[1], st));
    hipLaunchKernelGGL(semi_senone_kernel, dim3((unsigned)sen_blocks), dim3(256), 0, st, P);
    HIP_OK(hipGetLastError());
    if (m->sw.timing) {
        HIP_OK(hipEventRecord(m->sw.ev[2], st));
        m->sw.timing_pieced = 0;
    }
    return 0;
}
