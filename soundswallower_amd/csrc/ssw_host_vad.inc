/* ssw_host_vad.inc -- host: ssw_vad_batch, ssw_vad_debug_features, ssw_endpoint_batch (the
 * object, the host path and the endpointer's replay are ssw_vad.c).  The ssw_vad_t owns its
 * device workspace: the streams' states, the features of the last call, the offsets. */

static void
vad_dev_free(struct ssw_vad_s *v)
{
    (void)hipFree(v->d_state);
    (void)hipFree(v->d_feat);
    (void)hipFree(v->d_off);
    v->d_state = v->d_feat = v->d_off = NULL;
    v->d_state_cap = v->d_feat_cap = v->d_off_cap = 0;
}

static int
vad_reserve(void **p, size_t *cap, size_t bytes, const char *who)
{
    DevBuf b;
    b.p = (unsigned char *)*p;
    b.cap = *cap;
    const int rv = devbuf_reserve(b, bytes, who);
    *p = b.p;
    *cap = b.cap;
    return rv;
}

/* streams per workgroup: a lane per stream is one instruction stream whether 8 or 64 lanes of
 * its wave are in use, while staging costs a loop iteration per stream of the workgroup.  So a
 * batch is spread over the device's compute units first, and only a batch beyond 8 streams per
 * unit fills the waves further.  ssw_vad_set_streams_per_workgroup fixes the number instead. */
static int
vad_streams_per_workgroup(ssw_vad_t *v, int32_t n_streams)
{
    if (v->spw != 0)
        return v->spw;
    if (v->n_cus == 0) {
        int dev = 0, n = 0;
        v->n_cus = 256;
        if (hipGetDevice(&dev) == hipSuccess
            && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            v->n_cus = n;
    }
    int spw = 8;
    while (spw < 64 && (int64_t)spw * v->n_cus < n_streams)
        spw *= 2;
    return spw;
}

extern "C" int
ssw_vad_batch(ssw_vad_t *v, const int16_t *d_pcm, const int64_t *samp_off, int32_t n_streams,
              int8_t *d_is_speech, int32_t *frame_off_out, ssw_vad_state_t *state, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (ssw_vad_frame_offsets(v, samp_off, n_streams, frame_off_out) < 0)
        return -1;
    const int64_t total = frame_off_out[n_streams];
    if (total > 0 && (d_pcm == NULL || d_is_speech == NULL)) {
        ssw_set_error("ssw_vad_batch: bad arguments");
        return -1;
    }
    v->feat_frames = -1;
    v->dev_free = vad_dev_free;
    if (n_streams == 0) {
        v->feat_frames = 0;
        return 0;
    }
    const size_t off64 = align256(sizeof(int64_t) * ((size_t)n_streams + 1));
    const size_t off_bytes = off64 + sizeof(int32_t) * ((size_t)n_streams + 1);
    if (vad_reserve(&v->d_state, &v->d_state_cap, sizeof(ssw_vad_state_t) * (size_t)n_streams,
                    "ssw_vad_batch (states)") < 0
        || vad_reserve(&v->d_feat, &v->d_feat_cap, sizeof(int16_t) * 7 * (size_t)std::max<int64_t>(total, 1),
                       "ssw_vad_batch (features)") < 0
        || vad_reserve(&v->d_off, &v->d_off_cap, off_bytes, "ssw_vad_batch (offsets)") < 0)
        return -1;
    unsigned char *d_off = (unsigned char *)v->d_off;
    HIP_OK(hipMemcpyAsync(d_off, samp_off, sizeof(int64_t) * ((size_t)n_streams + 1),
                          hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_off + off64, frame_off_out, sizeof(int32_t) * ((size_t)n_streams + 1),
                          hipMemcpyHostToDevice, st));
    if (state != NULL)
        HIP_OK(hipMemcpyAsync(v->d_state, state, sizeof(ssw_vad_state_t) * (size_t)n_streams,
                              hipMemcpyHostToDevice, st));
    VadParams P;
    memset(&P, 0, sizeof(P));
    P.pcm = d_pcm;
    P.samp_off = (const int64_t *)d_off;
    P.frame_off = (const int32_t *)(d_off + off64);
    P.is_speech = d_is_speech;
    P.feat = (int16_t *)v->d_feat;
    P.state = (ssw_vad_state_t *)v->d_state;
    P.n_streams = n_streams;
    P.spw = vad_streams_per_workgroup(v, n_streams);
    P.fresh = state == NULL;
    P.frame_size = v->frame_size;
    P.nb_len = v->nb_len;
    P.th.overhead1 = v->overhead1;
    P.th.overhead2 = v->overhead2;
    P.th.individual = v->individual;
    P.th.total = v->total;
    const size_t lds = vad_lds_bytes();
    void (*kern)(const VadParams) = v->closest_rate == 8000    ? vad_batch_kernel<8000>
                                    : v->closest_rate == 16000 ? vad_batch_kernel<16000>
                                    : v->closest_rate == 32000 ? vad_batch_kernel<32000>
                                                               : vad_batch_kernel<48000>;
    HIP_OK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_streams + P.spw - 1) / P.spw)), dim3(VAD_LANES),
                       lds, st, P);
    HIP_OK(hipGetLastError());
    if (state != NULL)
        HIP_OK(hipMemcpyAsync(state, v->d_state, sizeof(ssw_vad_state_t) * (size_t)n_streams,
                              hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    v->feat_frames = total;
    return 0;
}

extern "C" int
ssw_vad_debug_features(ssw_vad_t *v, int16_t *out, int64_t n_frames)
{
    if (v == NULL || v->feat_frames < 0 || n_frames != v->feat_frames || (n_frames > 0 && out == NULL)) {
        ssw_set_error("ssw_vad_debug_features: no ssw_vad_batch call of %lld frames to show",
                      (long long)n_frames);
        return -1;
    }
    if (n_frames > 0)
        HIP_OK(hipMemcpy(out, v->d_feat, sizeof(int16_t) * 7 * (size_t)n_frames, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" ssw_endpoints_t *
ssw_endpoint_batch(ssw_vad_t *v, double window, double ratio, const int16_t *d_pcm,
                   const int64_t *samp_off, int32_t n_streams, void *stream)
{
    if (v == NULL || samp_off == NULL || n_streams < 0) {
        ssw_set_error("ssw_endpoint_batch: bad arguments");
        return NULL;
    }
    std::vector<int32_t> frame_off((size_t)n_streams + 1, 0);
    std::vector<int64_t> tail((size_t)n_streams, 0);
    if (ssw_vad_frame_offsets(v, samp_off, n_streams, frame_off.data()) < 0)
        return NULL;
    /* (the window and the ratio are refused before any device work) */
    {
        const int8_t none = 0;
        const int64_t zero = 0;
        const int32_t fo[2] = { 0, 0 };
        ssw_endpoints_t *probe = ssw_endpoints_replay(v, window, ratio, &none, fo, &zero, 1);
        if (probe == NULL)
            return NULL;
        ssw_endpoints_free(probe);
    }
    const size_t total = (size_t)frame_off[n_streams];
    std::vector<int8_t> dec(std::max<size_t>(total, 1));
    int8_t *d_dec = NULL;
    if (hipMalloc((void **)&d_dec, std::max<size_t>(total, 1)) != hipSuccess) {
        (void)hipGetLastError();
        ssw_set_error("ssw_endpoint_batch: %zu bytes of device memory", total);
        return NULL;
    }
    int rv = ssw_vad_batch(v, d_pcm, samp_off, n_streams, d_dec, frame_off.data(), NULL, stream);
    if (rv == 0 && total > 0 && hipMemcpy(dec.data(), d_dec, total, hipMemcpyDeviceToHost) != hipSuccess) {
        ssw_set_error("ssw_endpoint_batch: the decisions could not be copied to the host");
        rv = -1;
    }
    (void)hipFree(d_dec);
    if (rv < 0)
        return NULL;
    for (int32_t u = 0; u < n_streams; ++u)
        tail[u] = (samp_off[u + 1] - samp_off[u]) % v->frame_size;
    return ssw_endpoints_replay(v, window, ratio, dec.data(), frame_off.data(), tail.data(), n_streams);
}
