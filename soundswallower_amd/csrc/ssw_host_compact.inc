/* ssw_host_compact.inc -- host: compact score rows for batches whose alignments are known before
 * they are scored (BASELINE configs 3 and 5: phone strings given; the second pass of
 * decoder_alignment: phones from alignment_populate).  ssw_compact_plan_create /
 * ssw_score_batch_compact / ssw_align_batch_compact; kernels in ssw_k6_compact.inc and the
 * COMPACT instances of ptm_senone_kernel.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */

extern "C" ssw_compact_plan_t *
ssw_compact_plan_create(ssw_model_t *m, int32_t n_utts, const int32_t *frame_off,
                        const int32_t *phone_off, const uint16_t *senid, void *stream)
{
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    if (m->device == SSW_DEVICE_NONE) {
        ssw_set_error("model was loaded with device = SSW_DEVICE_NONE (tables only)");
        return NULL;
    }
    if (n_utts <= 0 || frame_off == NULL || phone_off == NULL || senid == NULL || frame_off[0] != 0
        || phone_off[0] != 0) {
        ssw_set_error("ssw_compact_plan_create: bad arguments");
        return NULL;
    }
    if (h->sc_rec != NULL && semi_refuse(SSW_SCORER_S2_SEMI, "ssw_compact_plan_create") < 0)
        return NULL; /* a single-codebook model */
    if (cont_refuse(m, "ssw_compact_plan_create") < 0)
        return NULL;
    if (h->n_emit_state != 3 || m->d_sen_slot == NULL) {
        ssw_set_error("ssw_compact_plan_create: 3-state models with mixture weights only");
        return NULL;
    }
    ssw_compact_plan_s *p = new ssw_compact_plan_s();
    p->m = m;
    p->n_utts = n_utts;
    p->n_frames = frame_off[n_utts];
    p->total_phones = phone_off[n_utts];
    p->frame_off.assign(frame_off, frame_off + n_utts + 1);
    p->phone_off.assign(phone_off, phone_off + n_utts + 1);
    p->cstride.resize((size_t)n_utts);
    p->crow_off.resize((size_t)n_utts);
    p->d_mem = NULL;
    size_t elems = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int nf = frame_off[u + 1] - frame_off[u], np = phone_off[u + 1] - phone_off[u];
        if (nf < 0 || np < 1) {
            ssw_set_error("utterance %d: %d phones, %d frames", u, np, nf);
            delete p;
            return NULL;
        }
        /* (the alignment kernels' per-state row indices are uint16) */
        if (3 * (size_t)np * 2 > 0xfffe) {
            ssw_set_error("utterance %d: %d phones are more than a compact row holds (10,922: "
                          "its per-state row indices are 16 bits); full rows -- ssw_score_batch "
                          "+ ssw_align_batch, compallsen = yes -- take any length", u, np);
            delete p;
            return NULL;
        }
        p->cstride[(size_t)u] = (3 * np + 1) & ~1; /* even: rows stay 4-byte aligned */
        p->crow_off[(size_t)u] = (long long)elems;
        elems += (size_t)nf * (size_t)p->cstride[(size_t)u];
    }
    for (size_t i = 0; i < (size_t)p->total_phones * 3; ++i)
        if (senid[i] >= h->n_sen) {
            ssw_set_error("phone %zu: senone %d of %d", i / 3, senid[i], h->n_sen);
            delete p;
            return NULL;
        }
    p->elems = elems;
    /* one device allocation, every table at a 256-byte boundary */
    WsLayout L;
    const size_t nst = (size_t)p->total_phones * 3;
    const size_t o_fo = L.out(sizeof(int32_t) * ((size_t)n_utts + 1));
    const size_t o_po = L.out(sizeof(int32_t) * ((size_t)n_utts + 1));
    const size_t o_cs = L.out(sizeof(int32_t) * (size_t)n_utts);
    const size_t o_ro = L.out(sizeof(long long) * (size_t)n_utts);
    const size_t o_uf = L.out(sizeof(int32_t) * (size_t)std::max(p->n_frames, 1));
    const size_t o_sid = L.out(sizeof(uint16_t) * nst + 16);
    const size_t o_cidx = L.out(sizeof(uint16_t) * nst + 16);
    const size_t o_cpos = L.out(sizeof(uint32_t) * (size_t)n_utts * (size_t)m->slot_stride);
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess)
        e = hipMalloc((void **)&p->d_mem, L.size());
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ssw_set_error("ssw_compact_plan_create: %zu bytes of device memory: %s", L.size(),
                      hipGetErrorString(e));
        delete p;
        return NULL;
    }
    p->d_frame_off = reinterpret_cast<int32_t *>(p->d_mem + o_fo);
    p->d_phone_off = reinterpret_cast<int32_t *>(p->d_mem + o_po);
    p->d_cstride = reinterpret_cast<int32_t *>(p->d_mem + o_cs);
    p->d_crow_off = reinterpret_cast<long long *>(p->d_mem + o_ro);
    p->d_utt_of_frame = reinterpret_cast<int32_t *>(p->d_mem + o_uf);
    p->d_senid = reinterpret_cast<uint16_t *>(p->d_mem + o_sid);
    p->d_cidx = reinterpret_cast<uint16_t *>(p->d_mem + o_cidx);
    p->d_cpos = reinterpret_cast<uint32_t *>(p->d_mem + o_cpos);
    /* (the host vectors live as long as the plan: asynchronous copies may read them later) */
    e = hipMemcpyAsync(p->d_frame_off, p->frame_off.data(), sizeof(int32_t) * ((size_t)n_utts + 1),
                       hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->d_phone_off, p->phone_off.data(), sizeof(int32_t) * ((size_t)n_utts + 1),
                           hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->d_cstride, p->cstride.data(), sizeof(int32_t) * (size_t)n_utts,
                           hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->d_crow_off, p->crow_off.data(), sizeof(long long) * (size_t)n_utts,
                           hipMemcpyHostToDevice, st);
    if (e == hipSuccess) /* the caller's array: copied before this call returns (synchronise below) */
        e = hipMemcpyAsync(p->d_senid, senid, sizeof(uint16_t) * nst, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        CompactPlanParams C;
        C.senid = p->d_senid;
        C.phone_off = p->d_phone_off;
        C.sen_slot = m->d_sen_slot;
        C.cpos = p->d_cpos;
        C.cidx = p->d_cidx;
        C.slot_stride = m->slot_stride;
        C.n_sen = h->n_sen;
        const size_t lds = sizeof(uint32_t) * (size_t)m->slot_stride;
        C.in_lds = lds <= 64 * 1024;
        hipLaunchKernelGGL(compact_plan_kernel, dim3((unsigned)n_utts), dim3(256),
                           C.in_lds ? lds : 0, st, C);
        if (p->n_frames > 0)
            hipLaunchKernelGGL(utt_of_frame_kernel, dim3((unsigned)((p->n_frames + 255) / 256)),
                               dim3(256), 0, st, p->d_frame_off, n_utts, p->n_frames,
                               p->d_utt_of_frame);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st); /* senid is the caller's to reuse */
    if (e != hipSuccess) {
        ssw_set_error("ssw_compact_plan_create: %s", hipGetErrorString(e));
        (void)hipFree(p->d_mem);
        delete p;
        return NULL;
    }
    return p;
}

extern "C" void
ssw_compact_plan_free(ssw_compact_plan_t *p)
{
    if (p == NULL)
        return;
    (void)hipFree(p->d_mem);
    delete p;
}

extern "C" size_t
ssw_compact_plan_elems(const ssw_compact_plan_t *p)
{
    return p->elems;
}

/* where utterance u's rows are in the compact buffer (int16 elements) and how long a row is */
extern "C" int
ssw_compact_plan_rows(const ssw_compact_plan_t *p, int32_t utt, long long *row_off, int32_t *stride)
{
    if (utt < 0 || utt >= p->n_utts) {
        ssw_set_error("ssw_compact_plan_rows: utterance %d of %d", utt, p->n_utts);
        return -1;
    }
    if (row_off != NULL)
        *row_off = p->crow_off[(size_t)utt];
    if (stride != NULL)
        *stride = p->cstride[(size_t)utt];
    return 0;
}

extern "C" int
ssw_score_batch_compact(ssw_model_t *m, int scorer, const float *d_feats,
                        const ssw_compact_plan_t *plan, int16_t *d_compact, void *stream,
                        uint32_t flags)
{
    if (semi_refuse(scorer, "ssw_score_batch_compact") < 0
        || cont_refuse(m, "ssw_score_batch_compact") < 0)
        return -1;
    if (plan == NULL || plan->m != m) {
        ssw_set_error("ssw_score_batch_compact: the plan belongs to another model");
        return -1;
    }
    if (plan->n_frames == 0)
        return 0;
    if (d_compact == NULL || d_feats == NULL) {
        ssw_set_error("ssw_score_batch_compact: NULL buffer");
        return -1;
    }
    /* before the knobs and the fall-back's workspace are touched: a second thread on the same
     * model gets the documented "model is in use" error, not a freed workspace (ADVICE r5;
     * score_batch_impl takes the guard again -- nesting on one thread is allowed) */
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    refresh_knobs(m);
    /* launches without a COMPACT instance: full rows into a workspace, then a gather */
    bool direct = scorer == SSW_SCORER_PTM;
    if (scorer == SSW_SCORER_MS) {
        /* the smallest senone launch of the call: the batch, or the last piece of a batch that
         * score_batch_impl cuts (same arithmetic as there) */
        int least = plan->n_frames;
        const int piece = m->kn.score_piece;
        const bool mfma = m->d_wfrag != NULL && h->n_feat * 13 == h->veclen_total
            && plan->n_frames >= m->kn.mfma_min_frames && !m->kn.scan_fma;
        if (mfma && piece > 0 && plan->n_frames >= 2 * piece) {
            const int n_pieces = (plan->n_frames + piece / 2) / piece;
            const int len = ((plan->n_frames + n_pieces - 1) / n_pieces + 255) / 256 * 256;
            least = plan->n_frames - (plan->n_frames - 1) / len * len;
            least = least < len ? least : len;
        }
        direct = ms_takes_packed_kernel(m, least);
    }
    ScoreReq R{};
    R.scorer = scorer;
    R.d_feats = d_feats;
    R.n_frames = plan->n_frames;
    R.utt_off = plan->frame_off.data();
    R.n_utts = plan->n_utts;
    R.stream = stream;
    R.flags = flags & SSW_SCORE_SHARE_DEVICE;
    if (direct) {
        R.d_out = d_compact;
        R.cp = plan;
        return score_batch_impl(m, R);
    }
    HIP_OK(hipSetDevice(m->device));
    if (devbuf_reserve(m->full_tmp, sizeof(int16_t) * (size_t)plan->n_frames * h->n_sen,
                       "ssw_score_batch_compact") < 0)
        return -1;
    R.d_out = m->full_tmp.as<int16_t>();
    if (score_batch_impl(m, R) < 0)
        return -1;
    CompactGatherParams G;
    G.full = m->full_tmp.as<int16_t>();
    G.utt_of_frame = plan->d_utt_of_frame;
    G.cutt_off = plan->d_frame_off;
    G.cstride = plan->d_cstride;
    G.phone_off = plan->d_phone_off;
    G.crow_off = plan->d_crow_off;
    G.senid = plan->d_senid;
    G.out = d_compact;
    G.n_sen = h->n_sen;
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)plan->n_frames), dim3(256), 0,
                       (hipStream_t)stream, G);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int
ssw_align_batch_compact(ssw_model_t *m, const ssw_compact_plan_t *plan, const int16_t *d_compact,
                        const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                        ssw_align_entry_t *state_io, int32_t *status, void *stream, uint32_t flags)
{
    if (plan == NULL || plan->m != m) {
        ssw_set_error("ssw_align_batch_compact: the plan belongs to another model");
        return -1;
    }
    ModelBusy busy_(m); /* (held here already: the flag below belongs to this call) */
    if (!busy_.ok)
        return -1;
    struct Flag {
        ssw_model_s *m;
        ~Flag() { m->align_state_out_only = 0; }
    } flag_{ m };
    m->align_state_out_only = (flags & SSW_ALIGN_STATE_OUT_ONLY) ? 1 : 0;
    /* (senid: only its non-NULL-ness is looked at on this path -- the per-state row indices
     * come from the plan) */
    static const uint16_t dummy = 0;
    return align_batch_levels(m, d_compact, plan->n_utts, plan->frame_off.data(),
                              plan->phone_off.data(), &dummy, tmatid, sf, ef, state_io, status,
                              stream, plan);
}
