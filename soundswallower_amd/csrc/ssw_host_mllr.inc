/* ssw_host_mllr.inc -- host: MLLR speaker adaptation of a loaded model.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order).
 * Launches no kernel: the transform and the table rebuild run on the host
 * (ssw_model.c:ssw_host_model_apply_mllr, where the double-precision log of the variance
 * precomputation is the libm call the reference makes); this file copies the rebuilt tables into
 * the allocations upload_model made. */

/* The Gaussian tables of upload_model once more, sizes unchanged, nothing allocated.  Mixture
 * weights, sen2cb, the slot layout, the transition matrices and the log-add tables do not depend
 * on the Gaussians and stay.  d_wfrag == NULL with host fragments = the matrix-core self-test
 * failed at load: it is about the device, not the model, and stays failed. */
static int
reupload_gaussians(ssw_model_s *m)
{
    const ssw_host_model_t *h = m->h;
    const size_t ncbf = (size_t)m->n_cbf;
    if (h->sc_rec != NULL)
        HIP_OK(hipMemcpy(m->d_sc_rec, h->sc_rec,
                         (size_t)h->n_feat * SSW_SC_ROWS * SSW_SC_MAX_DENSITY * sizeof(float),
                         hipMemcpyHostToDevice));
    if (h->cont_rec != NULL)
        HIP_OK(hipMemcpy(m->d_cont_rec, h->cont_rec, h->cont_floats * sizeof(float),
                         hipMemcpyHostToDevice));
    if (h->cont_rec_sm != NULL && m->d_cont_rec_sm != NULL) /* (ssw_model_enable_active) */
        HIP_OK(hipMemcpy(m->d_cont_rec_sm, h->cont_rec_sm, h->cont_sm_floats * sizeof(float),
                         hipMemcpyHostToDevice));
    if (h->rec != NULL) {
        const size_t nrec = ncbf * h->n_density * SSW_REC_FLOATS;
        const size_t nd0 = ncbf * SSW_REC_FLOATS, nex = ncbf * SSW_EXLIST_STRIDE;
        m->n_exact_form = h->n_exact_form;
        HIP_OK(hipMemcpy(m->d_rec, h->rec, nrec * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(m->d_recq, h->recq, nrec * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(m->d_recmax, h->recd0, nd0 * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(m->d_exlist, h->exlist, nex * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (h->wfrag != NULL && m->d_rec28 != NULL) {
            if (m->d_wfrag != NULL)
                HIP_OK(hipMemcpy(m->d_wfrag, h->wfrag,
                                 ncbf * SSW_WFRAG_PER_CBF * sizeof(uint16_t), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->d_rec28, h->rec28, ncbf * h->n_density * 28 * sizeof(float),
                             hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->d_exlistm, h->exlistm, nex * sizeof(uint32_t),
                             hipMemcpyHostToDevice));
        }
    }
    return 0;
}

extern "C" int
ssw_model_apply_mllr(ssw_model_t *m, const ssw_mllr_t *mllr)
{
    if (m == NULL) {
        ssw_set_error("ssw_model_apply_mllr: NULL model");
        return -1;
    }
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    /* (a refused transform ends here: host tables and device untouched) */
    const double t0 = now_ms();
    if (ssw_host_model_apply_mllr(m->h, mllr) < 0)
        return -1;
    const double t1 = now_ms();
    m->mllr_ms[0] = (float)(t1 - t0);
    m->mllr_ms[1] = 0.0f;
    if (m->device == SSW_DEVICE_NONE)
        return 0;
    /* launches still reading the device tables finish first: the copies are blocking, but on
     * the null stream, and a caller's non-blocking stream would not wait for them */
    HIP_OK(hipSetDevice(m->device));
    HIP_OK(hipDeviceSynchronize());
    if (reupload_gaussians(m) < 0)
        return -1;
    /* what refers to scores of the parameters before */
    m->sw.last_n_frames = 0;
    m->sw.stats_pending = 0;
    m->mllr_ms[1] = (float)(now_ms() - t1);
    return 0;
}

extern "C" int
ssw_model_mllr_timing(const ssw_model_t *m, float ms[2])
{
    if (m == NULL || ms == NULL)
        return -1;
    ms[0] = m->mllr_ms[0];
    ms[1] = m->mllr_ms[1];
    return 0;
}

extern "C" int
ssw_model_mllr_generation(const ssw_model_t *m)
{
    return m != NULL ? m->h->mllr_generation : 0;
}
