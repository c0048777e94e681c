/* ssw_host_active.inc -- host: the reference's DEFAULT configuration (compallsen = no) for a
 * batch: state_align_search over senone scores that acmod computes for the active senones only
 * (src/acmod.c:822-999, src/ptm_mgau.c:264-403, src/state_align_search.c:177-213).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */

/* (active_first_frames and ActiveSetBuilder: ssw_active_set.inc) */

/* one utterance's segments, built by a host thread of its own */
struct ActiveUtt {
    std::vector<uint32_t> real_ent, bridge_ent; /* real_ent sorted by slot, real_rank beside it */
    std::vector<uint16_t> real_rank;
    std::vector<int32_t> seg_start, seg_nreal, seg_nbridge; /* per segment: first frame (in the
                                                             * utterance), prefix, bridge count */
    std::vector<unsigned long long> seg_cbmask;
    int cap, err;
    char msg[200];
};

struct ActiveJob {
    const ssw_host_model_t *h;
    const uint16_t *sen_slot;
    int n_utts;
    const int32_t *frame_off, *phone_off, *sf, *ef;
    const uint16_t *senid;
    const uint32_t *seed_active;
    ActiveUtt *out;
    int per_chunk;
};

static void
active_build_chunk(void *arg, int chunk)
{
    const ActiveJob *J = static_cast<const ActiveJob *>(arg);
    const ssw_host_model_t *h = J->h;
    const int vec_words = (h->n_sen + 31) / 32;
    std::vector<int32_t> first;
    const int u0 = chunk * J->per_chunk, u1 = std::min(J->n_utts, u0 + J->per_chunk);
    for (int u = u0; u < u1; ++u) {
        ActiveUtt &A = J->out[u];
        A.cap = 1;
        A.err = 0;
        const int f0 = J->frame_off[u], nf = J->frame_off[u + 1] - f0;
        const int p0 = J->phone_off[u], np = J->phone_off[u + 1] - p0;
        (void)f0;
        if (nf < 0 || np < 1) {
            A.err = 1;
            snprintf(A.msg, sizeof(A.msg), "utterance %d: %d phones, %d frames", u, np, nf);
            continue;
        }
        bool bad = false;
        for (int p = p0 * 3; p < (p0 + np) * 3 && !bad; ++p)
            if (J->senid[p] >= h->n_sen) {
                A.err = 1;
                snprintf(A.msg, sizeof(A.msg), "phone %d: senone %d of %d", p / 3, J->senid[p], h->n_sen);
                bad = true;
            }
        if (bad)
            continue;
        if (active_first_frames(J->sf + p0, J->ef + p0, np, nf, first) < 0) {
            A.err = 2; /* (the message is in this thread's error slot: repeated by the caller) */
            snprintf(A.msg, sizeof(A.msg), "%s", ssw_last_error());
            continue;
        }
        auto entry_of = [&](int sen) {
            return (uint32_t)J->sen_slot[(size_t)sen] | ((uint32_t)h->sen2cb[sen] << 16);
        };
        ActiveSetBuilder B(h->n_sen);
        unsigned long long mask_real = 0;
        size_t emitted = 0;
        if (J->seed_active != NULL) /* what the first pass left active, ascending */
            for (int wd = 0; wd < vec_words; ++wd) {
                uint32_t bits = J->seed_active[(size_t)u * vec_words + wd];
                while (bits) {
                    const int sen = wd * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (sen < h->n_sen)
                        B.insert(sen);
                }
            }
        int next_phone = 0;
        for (int t = 0; t < nf;) {
            /* phones entered by frame t join the set; the set then holds until the next entry */
            while (next_phone < np && first[next_phone] <= t) {
                for (int j = 0; j < 3; ++j)
                    B.insert(J->senid[(size_t)(p0 + next_phone) * 3 + j]);
                ++next_phone;
            }
            const int t_end = next_phone < np && first[next_phone] < nf ? first[next_phone] : nf;
            for (; emitted < B.order.size(); ++emitted)
                mask_real |= 1ull << h->sen2cb[B.order[emitted]];
            unsigned long long mask = mask_real;
            for (int b : B.bridges) {
                A.bridge_ent.push_back(entry_of(b));
                mask |= 1ull << h->sen2cb[b];
            }
            A.seg_start.push_back(t);
            A.seg_nreal.push_back((int32_t)B.order.size());
            A.seg_nbridge.push_back((int32_t)B.bridges.size());
            A.seg_cbmask.push_back(mask);
            t = t_end;
        }
        /* the utterance's real senones by slot, each with its rank in the order of listing */
        {
            std::vector<uint64_t> key(B.order.size());
            for (size_t r = 0; r < B.order.size(); ++r)
                key[r] = ((uint64_t)entry_of(B.order[r]) & 0xffffull) << 48
                    | (uint64_t)entry_of(B.order[r]) << 16 | (uint64_t)r;
            std::sort(key.begin(), key.end());
            A.real_ent.resize(key.size());
            A.real_rank.resize(key.size());
            for (size_t k = 0; k < key.size(); ++k) {
                A.real_ent[k] = (uint32_t)(key[k] >> 16);
                A.real_rank[k] = (uint16_t)(key[k] & 0xffffu);
            }
            int max_b = 0;
            for (int nb : A.seg_nbridge)
                max_b = std::max(max_b, nb);
            A.cap = std::max(1, (int)B.order.size() + max_b);
        }
    }
}

extern "C" int
ssw_align_batch_active(ssw_model_t *m, const float *d_feats, int32_t n_utts,
                       const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                       const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                       const uint32_t *seed_active, ssw_align_entry_t *state_io, int32_t *status,
                       int16_t *d_senscr, void *stream)
{
    return ssw_align_batch_active_ex(m, SSW_SCORER_PTM, d_feats, n_utts, frame_off, phone_off, senid,
                                     tmatid, sf, ef, seed_active, state_io, status, d_senscr, stream);
}

static int
align_batch_active_impl(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_utts,
                        const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                        const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                        const uint32_t *seed_active, ssw_align_entry_t *state_io, int32_t *status,
                        int16_t *d_senscr, void *stream, const uint32_t *d_carry_rows);

extern "C" int
ssw_align_batch_active_ex(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_utts,
                          const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                          const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                          const uint32_t *seed_active, ssw_align_entry_t *state_io, int32_t *status,
                          int16_t *d_senscr, void *stream)
{
    return align_batch_active_impl(m, scorer, d_feats, n_utts, frame_off, phone_off, senid, tmatid, sf,
                                   ef, seed_active, state_io, status, d_senscr, stream, NULL);
}

/* d_carry_rows: NULL (every utterance from the reset history), or device uint32 [n_utts][n_cbf]:
 * the order each utterance's frame 0 starts from (ssw_align_text_batch_active with
 * two_pass_history: what its first pass left in history slot 1) */
static int
align_batch_active_impl(ssw_model_t *m, int scorer, const float *d_feats, int32_t n_utts,
                        const int32_t *frame_off, const int32_t *phone_off, const uint16_t *senid,
                        const int16_t *tmatid, const int32_t *sf, const int32_t *ef,
                        const uint32_t *seed_active, ssw_align_entry_t *state_io, int32_t *status,
                        int16_t *d_senscr, void *stream, const uint32_t *d_carry_rows)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    const ssw_host_model_t *h = m->h;
    hipStream_t st = (hipStream_t)stream;
    if (semi_refuse(scorer, "ssw_align_batch_active") < 0
        || cont_refuse_active(m, "ssw_align_batch_active") < 0)
        return -1;
    if (n_utts <= 0)
        return 0;
    if (check_scorer_shape(m, scorer) < 0)
        return -1;
    if ((h->n_cb > 64 && !h->continuous) || h->n_emit_state != 3) {
        ssw_set_error("ssw_align_batch_active: built for <= 64 codebooks and 3-state HMMs");
        return -1;
    }
    /* (score_batch_impl's refusal, said here before the plan, the uploads and any launch) */
    if (h->cfg.ds != 1 || m->force_exact) {
        ssw_set_error("active-set batches: ds = 1 only");
        return -1;
    }
    if (!d_feats || !frame_off || !phone_off || !senid || !tmatid || !sf || !ef || !state_io
        || !status || frame_off[0] != 0 || phone_off[0] != 0) {
        ssw_set_error("ssw_align_batch_active: bad arguments");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    if (h->continuous) /* bitmap rows and the listed-senone kernel, no compact plan */
        return cont_align_active(m, d_feats, n_utts, frame_off, phone_off, senid, tmatid, sf, ef,
                                 seed_active, state_io, status, d_senscr, stream);
    const int n_frames = frame_off[n_utts];
    /* slot of every senone: the device table's host twin (upload_model) */
    const uint16_t *sen_slot = m->h_sen_slot;
    /* segments (runs of frames that share their active set), utterance by utterance on the
     * host threads, then laid end to end */
    std::vector<ActiveUtt> per_utt((size_t)n_utts);
    {
        ActiveJob J;
        J.h = h;
        J.sen_slot = sen_slot;
        J.n_utts = n_utts;
        J.frame_off = frame_off;
        J.phone_off = phone_off;
        J.sf = sf;
        J.ef = ef;
        J.senid = senid;
        J.seed_active = seed_active;
        J.out = per_utt.data();
        J.per_chunk = std::max(1, (n_utts + 4 * ssw_host_threads() - 1) / (4 * ssw_host_threads()));
        ssw_parallel_for((n_utts + J.per_chunk - 1) / J.per_chunk, active_build_chunk, &J);
    }
    std::vector<int32_t> seg_of_frame((size_t)std::max(n_frames, 1));
    std::vector<int32_t> seg_utt, seg_nreal, seg_boff(1, 0), utt_real_off((size_t)n_utts + 1, 0);
    std::vector<uint32_t> real_ent, bridge_ent;
    std::vector<uint16_t> real_rank;
    std::vector<unsigned long long> seg_cbmask;
    int cap = 1;
    for (int u = 0; u < n_utts; ++u) {
        const ActiveUtt &A = per_utt[(size_t)u];
        if (A.err != 0) {
            ssw_set_error("%s", A.msg);
            return -1;
        }
        const int f0 = frame_off[u], nf = frame_off[u + 1] - f0;
        utt_real_off[(size_t)u] = (int32_t)real_ent.size();
        real_ent.insert(real_ent.end(), A.real_ent.begin(), A.real_ent.end());
        real_rank.insert(real_rank.end(), A.real_rank.begin(), A.real_rank.end());
        utt_real_off[(size_t)u + 1] = (int32_t)real_ent.size();
        bridge_ent.insert(bridge_ent.end(), A.bridge_ent.begin(), A.bridge_ent.end());
        cap = std::max(cap, A.cap);
        for (size_t k = 0; k < A.seg_start.size(); ++k) {
            const int seg = (int)seg_utt.size();
            const int t0 = A.seg_start[k], t1 = k + 1 < A.seg_start.size() ? A.seg_start[k + 1] : nf;
            seg_utt.push_back(u);
            seg_nreal.push_back(A.seg_nreal[k]);
            seg_boff.push_back(seg_boff.back() + A.seg_nbridge[k]);
            seg_cbmask.push_back(A.seg_cbmask[k]);
            for (int tt = t0; tt < t1; ++tt)
                seg_of_frame[(size_t)f0 + tt] = seg;
        }
    }
    const size_t n_seg = seg_utt.size();
    /* the alignment's compact rows: the plan's tables serve the senone kernel and the alignment */
    ssw_compact_plan_t *plan = ssw_compact_plan_create(m, n_utts, frame_off, phone_off, senid, stream);
    if (plan == NULL)
        return -1;
    struct PlanGuard {
        ssw_compact_plan_t *p;
        ~PlanGuard() { ssw_compact_plan_free(p); }
    } guard_{ plan };
    /* device workspace: segment tables and the compact rows */
    WsLayout L;
    const size_t o_sof = L.out(sizeof(int32_t) * (size_t)std::max(n_frames, 1));
    const size_t o_su = L.out(sizeof(int32_t) * std::max(n_seg, (size_t)1));
    const size_t o_sn = L.out(sizeof(int32_t) * std::max(n_seg, (size_t)1));
    const size_t o_sb = L.out(sizeof(int32_t) * (n_seg + 1));
    const size_t o_cm = L.out(sizeof(unsigned long long) * std::max(n_seg, (size_t)1));
    const size_t o_uo = L.out(sizeof(int32_t) * ((size_t)n_utts + 1));
    const size_t o_re = L.out(sizeof(uint32_t) * std::max(real_ent.size(), (size_t)1));
    const size_t o_rr = L.out(sizeof(uint16_t) * std::max(real_rank.size(), (size_t)1) + 16);
    const size_t o_be = L.out(sizeof(uint32_t) * std::max(bridge_ent.size(), (size_t)1));
    const size_t o_scr = L.out(sizeof(int16_t) * std::max(plan->elems, (size_t)1));
    if (devbuf_reserve(m->act_ws, L.size(), "ssw_align_batch_active") < 0)
        return -1;
    unsigned char *ws = m->act_ws.p;
    auto up = [&](size_t at, const void *src, size_t bytes) {
        return bytes == 0 ? hipSuccess : hipMemcpyAsync(ws + at, src, bytes, hipMemcpyHostToDevice, st);
    };
    HIP_OK(up(o_sof, seg_of_frame.data(), sizeof(int32_t) * (size_t)n_frames));
    HIP_OK(up(o_su, seg_utt.data(), sizeof(int32_t) * n_seg));
    HIP_OK(up(o_sn, seg_nreal.data(), sizeof(int32_t) * n_seg));
    HIP_OK(up(o_sb, seg_boff.data(), sizeof(int32_t) * (n_seg + 1)));
    HIP_OK(up(o_cm, seg_cbmask.data(), sizeof(unsigned long long) * n_seg));
    HIP_OK(up(o_uo, utt_real_off.data(), sizeof(int32_t) * ((size_t)n_utts + 1)));
    HIP_OK(up(o_re, real_ent.data(), sizeof(uint32_t) * real_ent.size()));
    HIP_OK(up(o_rr, real_rank.data(), sizeof(uint16_t) * real_rank.size()));
    HIP_OK(up(o_be, bridge_ent.data(), sizeof(uint32_t) * bridge_ent.size()));
    HIP_OK(hipStreamSynchronize(st)); /* the host vectors go out of scope before the kernels end */
    int16_t *d_compact = reinterpret_cast<int16_t *>(ws + o_scr);
    if (n_frames > 0) {
        SenoneActive2Params A;
        memset(&A, 0, sizeof(A));
        A.seg_of_frame = reinterpret_cast<const int32_t *>(ws + o_sof);
        A.seg_utt = reinterpret_cast<const int32_t *>(ws + o_su);
        A.seg_nreal = reinterpret_cast<const int32_t *>(ws + o_sn);
        A.seg_boff = reinterpret_cast<const int32_t *>(ws + o_sb);
        A.seg_cbmask = reinterpret_cast<const unsigned long long *>(ws + o_cm);
        A.utt_real_off = reinterpret_cast<const int32_t *>(ws + o_uo);
        A.real_ent = reinterpret_cast<const uint32_t *>(ws + o_re);
        A.real_rank = reinterpret_cast<const uint16_t *>(ws + o_rr);
        A.bridge_ent = reinterpret_cast<const uint32_t *>(ws + o_be);
        A.cpos = plan->d_cpos;
        A.crow_off = plan->d_crow_off;
        A.cstride = plan->d_cstride;
        A.cutt_off = plan->d_frame_off;
        A.out_c = d_compact;
        A.out_full = d_senscr;
        A.slot_sen = reinterpret_cast<const int16_t *>(m->d_slot_sen);
        A.cap = cap;
        ActiveSets act;
        act.seg_of_frame = A.seg_of_frame;
        act.seg_cbmask = A.seg_cbmask;
        act.a2 = &A;
        act.ls = NULL;
        act.row_of_frame = NULL;
        ScoreReq R{};
        R.scorer = scorer;
        R.d_feats = d_feats;
        R.n_frames = n_frames;
        R.utt_off = frame_off;
        R.n_utts = n_utts;
        R.d_out = d_compact;
        R.stream = stream;
        R.act = &act;
        R.d_carry_rows = d_carry_rows;
        if (score_batch_impl(m, R) < 0)
            return -1;
    }
    return align_batch_levels(m, d_compact, n_utts, frame_off, phone_off, senid, tmatid, sf, ef,
                              state_io, status, stream, plan);
}
