/* ssw_host_feat.inc -- host: ssw_feat_batch.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* dynamic features (SURVEY 8(f) row 2)                                                 */
/* ---------------------------------------------------------------------------------- */
extern "C" int
ssw_feat_batch(ssw_model_t *m, const float *d_cep, int32_t n_frames, const int32_t *utt_off,
               int32_t n_utts, int32_t ncep, float *d_out, void *stream)
{
    ModelBusy busy_(m);
    if (!busy_.ok)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    if (n_frames == 0 || n_utts == 0)
        return 0;
    if (check_has_device(m) < 0)
        return -1;
    if (ncep < 1 || ncep > 64 || n_frames < 0 || n_utts < 0 || utt_off == NULL
        || !utt_off_spans(utt_off, n_utts, n_frames)) {
        ssw_set_error("bad arguments to ssw_feat_batch");
        return -1;
    }
    HIP_OK(hipSetDevice(m->device));
    if (devbuf_reserve(m->feat_off, sizeof(int) * ((size_t)n_utts + 1), "ssw_feat_batch") < 0)
        return -1;
    int *d_off = m->feat_off.as<int>();
    hipError_t e = hipMemcpyAsync(d_off, utt_off, sizeof(int) * ((size_t)n_utts + 1),
                                  hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        FeatParams F;
        F.cep = d_cep;
        F.utt_off = d_off;
        F.out = d_out;
        F.n_utts = n_utts;
        F.ncep = ncep;
        hipLaunchKernelGGL(feat_1s_c_d_dd_kernel, dim3(n_utts), dim3(FEAT_THREADS), 0, st, F);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ssw_set_error("ssw_feat_batch: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}
