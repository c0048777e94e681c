/* ssw_vad.c -- host side of voice activity detection and endpointing: the ssw_vad_t object
 * (vad_init + vad_set_input_params, src/ps_vad.c:49-128), the host path ssw_vad_batch_host over
 * the arithmetic of ssw_vad_core.inc -- the source the kernel is built from too -- and the
 * endpointer's queue replayed over a decision array (src/ps_endpointer.c:53-322).  No HIP here:
 * a stand-alone host program can be built from this file alone. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

#define VAD_FN static inline
#define SSW_VAD_PITCH 1
#define VAD_UNROLL
#define VAD_NOUNROLL
#include "ssw_vad_core.inc"

/* WebRtcVad_set_mode_core's tables (vad_core.c:73-91): [mode][10, 20, 30 ms] */
static const int16_t k_overhang1[4][3] = { { 8, 4, 3 }, { 8, 4, 3 }, { 6, 3, 2 }, { 6, 3, 2 } };
static const int16_t k_overhang2[4][3] = { { 14, 7, 5 }, { 14, 7, 5 }, { 9, 5, 3 }, { 9, 5, 3 } };
static const int16_t k_local[4][3] = { { 24, 21, 24 }, { 37, 32, 37 }, { 82, 78, 82 }, { 94, 94, 94 } };
static const int16_t k_global[4][3] = { { 57, 48, 57 }, { 100, 80, 100 }, { 285, 260, 285 },
                                        { 1100, 1050, 1100 } };

ssw_vad_t *
ssw_vad_create(int32_t mode, int32_t sample_rate, double frame_length)
{
    static const int rates[4] = { 8000, 16000, 32000, 48000 };
    int i, closest = 0, ms, valid = 0, idx;
    double best_diff = 0.5;
    size_t frame_size;
    ssw_vad_t *v;
    if (mode < 0 || mode > 3) {
        ssw_set_error("Invalid VAD mode %d", mode);
        return NULL;
    }
    if (sample_rate == 0)
        sample_rate = 16000;
    if (frame_length == 0)
        frame_length = 0.03;
    for (i = 0; i < 4; ++i) {
        const double diff = fabs(1.0 - (double)rates[i] / sample_rate);
        if (diff < best_diff) {
            closest = rates[i];
            best_diff = diff;
        }
    }
    if (closest == 0) {
        ssw_set_error("No suitable sampling rate found for %d", sample_rate);
        return NULL;
    }
    if (!(frame_length > 0 && frame_length < 1)) { /* (keeps the product in a size_t's range) */
        ssw_set_error("Unsupported frame length %f", frame_length);
        return NULL;
    }
    frame_size = (size_t)(closest * frame_length);
    for (ms = 10; ms <= 30; ms += 10) /* WebRtcVad_ValidRateAndFrameLength */
        if (frame_size == (size_t)(closest / 1000 * ms))
            valid = ms;
    if (!valid) {
        ssw_set_error("Unsupported frame length %f", frame_length);
        return NULL;
    }
    v = (ssw_vad_t *)calloc(1, sizeof(*v));
    if (v == NULL) {
        ssw_set_error("ssw_vad_create: out of memory");
        return NULL;
    }
    v->mode = mode;
    v->sample_rate = sample_rate;
    v->closest_rate = closest;
    v->frame_size = (int32_t)frame_size;
    v->nb_len = 8 * valid;
    idx = valid / 10 - 1;
    v->overhead1 = k_overhang1[mode][idx];
    v->overhead2 = k_overhang2[mode][idx];
    v->individual = k_local[mode][idx];
    v->total = k_global[mode][idx];
    v->feat_frames = -1;
    return v;
}

void
ssw_vad_free(ssw_vad_t *v)
{
    if (v == NULL)
        return;
    if (v->dev_free)
        v->dev_free(v);
    free(v);
}

int32_t ssw_vad_frame_size(const ssw_vad_t *v) { return v ? v->frame_size : -1; }
int32_t ssw_vad_sample_rate(const ssw_vad_t *v) { return v ? v->sample_rate : -1; }
int32_t ssw_vad_closest_rate(const ssw_vad_t *v) { return v ? v->closest_rate : -1; }
double ssw_vad_frame_length(const ssw_vad_t *v) { return v ? (double)v->frame_size / v->sample_rate : 0; }

int
ssw_vad_set_streams_per_workgroup(ssw_vad_t *v, int32_t streams)
{
    if (v == NULL || !(streams == 0 || streams == 8 || streams == 16 || streams == 32 || streams == 64)) {
        ssw_set_error("ssw_vad_set_streams_per_workgroup: 0, 8, 16, 32 or 64");
        return -1;
    }
    v->spw = streams;
    return 0;
}

int64_t
ssw_vad_frame_count(const ssw_vad_t *v, int64_t n_samples)
{
    if (v == NULL || n_samples < 0) {
        ssw_set_error("ssw_vad_frame_count: bad arguments");
        return -1;
    }
    return n_samples / v->frame_size;
}

void
ssw_vad_state_init(ssw_vad_state_t *s)
{
    if (s != NULL)
        vad_core_init((int16_t *)s);
}

int
ssw_vad_frame_offsets(const ssw_vad_t *v, const int64_t *samp_off, int32_t n_streams,
                      int32_t *frame_off_out)
{
    int64_t total = 0;
    int32_t u;
    if (v == NULL || samp_off == NULL || frame_off_out == NULL || n_streams < 0) {
        ssw_set_error("vad batch: bad arguments");
        return -1;
    }
    frame_off_out[0] = 0;
    for (u = 0; u < n_streams; ++u) {
        const int64_t n = samp_off[u + 1] - samp_off[u];
        if (samp_off[u] < 0 || n < 0) {
            ssw_set_error("vad batch: samp_off must be non-negative and non-decreasing (stream %d)", u);
            return -1;
        }
        total += n / v->frame_size;
        if (total > INT32_MAX) {
            ssw_set_error("vad batch: more than 2^31 - 1 frames in one call");
            return -1;
        }
        frame_off_out[u + 1] = (int32_t)total;
    }
    return 0;
}

int
ssw_vad_batch_host(const ssw_vad_t *v, const int16_t *pcm, const int64_t *samp_off,
                   int32_t n_streams, int8_t *is_speech, int32_t *frame_off_out,
                   ssw_vad_state_t *state, int16_t *features)
{
    vad_thresholds_t th;
    int32_t u;
    if (ssw_vad_frame_offsets(v, samp_off, n_streams, frame_off_out) < 0)
        return -1;
    if (frame_off_out[n_streams] > 0 && (pcm == NULL || is_speech == NULL)) {
        ssw_set_error("ssw_vad_batch_host: bad arguments");
        return -1;
    }
    th.overhead1 = v->overhead1;
    th.overhead2 = v->overhead2;
    th.individual = v->individual;
    th.total = v->total;
    for (u = 0; u < n_streams; ++u) {
        int16_t w[VW_SLOTS];
        const int32_t n_frames = frame_off_out[u + 1] - frame_off_out[u];
        int32_t f;
        int i;
        if (state != NULL && state[u].initialised == 42)
            memcpy(w, &state[u], sizeof(state[u]));
        else
            vad_core_init(w);
        for (f = 0; f < n_frames; ++f) {
            /* (the core takes the audio through the pointer type it shares with the kernel) */
            int16_t *frame = (int16_t *)(pcm + samp_off[u] + (int64_t)f * v->frame_size);
            const int64_t row = (int64_t)frame_off_out[u] + f;
            if (v->closest_rate == 48000) {
                /* WebRtcVad_CalcVad48khz (vad_core.c:607-630): the frame's start every 10 ms */
                int rep;
                for (rep = 0; rep < v->frame_size / 480; ++rep)
                    vad_ingest(w, 48000, frame, 480, rep * 80);
            } else {
                vad_ingest(w, v->closest_rate, frame, v->frame_size, 0);
            }
            is_speech[row] = (int8_t)vad_decide(w, v->nb_len, th);
            if (features != NULL)
                for (i = 0; i < 7; ++i)
                    features[row * 7 + i] = w[VW_FEAT + i];
        }
        if (state != NULL)
            memcpy(&state[u], w, sizeof(state[u]));
    }
    return 0;
}

/* ---- the endpointer's queue over decisions ------------------------------------------------ */

typedef struct ep_s {
    int maxlen, start_frames, end_frames, frame_size, sample_rate;
    double frame_length;
    int8_t *is; /* [maxlen] */
    int pos, n, in_speech;
    double qstart_time, timestamp, speech_start, speech_end;
    int64_t qframes; /* frames that have left the queue's head: qstart_time's additions */
} ep_t;

/* a double as the int the reference's cast makes of it where that cast is defined; beyond the
 * int range (where the reference's behaviour is undefined) the nearest end, NaN as the low end */
static int
ep_int(double x)
{
    if (!(x > -1e9))
        return -1000000000;
    return x > 1e9 ? 1000000000 : (int)x;
}

/* endpointer_init's window arithmetic (src/ps_endpointer.c:63-81) */
static int
ep_configure(const ssw_vad_t *v, double window, double ratio, ep_t *ep)
{
    memset(ep, 0, sizeof(*ep));
    if (window == 0.0)
        window = 0.3;
    if (ratio == 0.0)
        ratio = 0.9;
    ep->frame_length = ssw_vad_frame_length(v);
    ep->frame_size = v->frame_size;
    ep->sample_rate = v->sample_rate;
    ep->maxlen = ep_int(window / ep->frame_length + 0.5);
    ep->start_frames = ep_int(ratio * ep->maxlen);
    ep->end_frames = ep_int((1.0 - ratio) * ep->maxlen + 0.5);
    if (ep->start_frames <= 0 || ep->start_frames >= ep->maxlen) {
        ssw_set_error("Ratio %.2f makes start-pointing stupid or impossible (%d frames of %d)",
                      ratio, ep->start_frames, ep->maxlen);
        return -1;
    }
    if (ep->end_frames <= 0 || ep->end_frames >= ep->maxlen) {
        ssw_set_error("Ratio %.2f makes end-pointing stupid or impossible (%d frames of %d)",
                      ratio, ep->end_frames, ep->maxlen);
        return -1;
    }
    return 0;
}

/* What ep_speech_count (:147-166) returns: the SUM of the stored classes over the slots its walk
 * visits.  Empty: none.  Full: every slot.  Between: the head slot, then the slots after it
 * round to the tail -- except that its first step does not wrap.  With the head in the last slot
 * the walk reads the byte PAST the array, skips slot 0 and goes on from slot 1.  That read is
 * undefined behaviour in the reference.  What it gets there: the array is calloc(1, maxlen), and
 * glibc zeroes a block to its usable size (8 mod 16 bytes), so the byte is 0 whenever maxlen is
 * not such a size; at maxlen 24, 40, 56, ... it would be the next block's header.  This replay
 * takes the byte as 0 for every maxlen. */
static int
ep_speech_count(const ep_t *ep)
{
    int count = 0, i;
    if (ep->n == 0)
        return 0;
    if (ep->n == ep->maxlen) {
        for (i = 0; i < ep->maxlen; ++i)
            count += ep->is[i];
        return count;
    }
    {
        const int tail = (ep->pos + ep->n) % ep->maxlen;
        const int past_the_end = 0;
        count = ep->is[ep->pos];
        if (ep->pos == ep->maxlen - 1) {
            count += past_the_end;
            i = 1;
        } else {
            i = ep->pos + 1;
        }
        for (; i != tail; i = (i + 1) % ep->maxlen)
            count += ep->is[i];
    }
    return count;
}

static void
ep_push(ep_t *ep, int is_speech)
{
    ep->is[(ep->pos + ep->n) % ep->maxlen] = (int8_t)is_speech;
    if (ep->n == ep->maxlen) {
        ep->qstart_time += ep->frame_length;
        ++ep->qframes;
        ep->pos = (ep->pos + 1) % ep->maxlen;
    } else {
        ep->n++;
    }
}

static int
ep_pop(ep_t *ep, int *out_is_speech)
{
    if (ep->n == 0)
        return 0;
    ep->qstart_time += ep->frame_length;
    ++ep->qframes;
    if (out_is_speech)
        *out_is_speech = ep->is[ep->pos];
    ep->pos = (ep->pos + 1) % ep->maxlen;
    ep->n--;
    return 1;
}

/* ep_linearize (:198-231): the whole array is rotated, stale entries included */
static void
ep_linearize(ep_t *ep, int8_t *tmp)
{
    if (ep->pos == 0)
        return;
    memcpy(tmp, ep->is, (size_t)ep->pos);
    memmove(ep->is, ep->is + ep->pos, (size_t)(ep->maxlen - ep->pos));
    memcpy(ep->is + (ep->maxlen - ep->pos), tmp, (size_t)ep->pos);
    ep->pos = 0;
}

typedef struct seg_list_s {
    ssw_endpoint_seg_t *segs;
    int32_t n, cap;
} seg_list_t;

static int
seg_push(seg_list_t *l, const ssw_endpoint_seg_t *s)
{
    if (l->n == l->cap) {
        const int32_t cap = l->cap ? 2 * l->cap : 64;
        ssw_endpoint_seg_t *p = (ssw_endpoint_seg_t *)realloc(l->segs, sizeof(*p) * (size_t)cap);
        if (p == NULL)
            return -1;
        l->segs = p;
        l->cap = cap;
    }
    l->segs[l->n++] = *s;
    return 0;
}

/* endpointer_process per decision, then endpointer_end_stream (:233-322) */
static int
ep_replay(ep_t *ep, const int8_t *is_speech, int64_t n_frames, int64_t tail, int8_t *tmp,
          seg_list_t *out)
{
    ssw_endpoint_seg_t seg;
    int64_t f;
    memset(ep->is, 0, (size_t)ep->maxlen);
    ep->pos = ep->n = ep->in_speech = 0;
    ep->qstart_time = ep->timestamp = ep->speech_start = ep->speech_end = 0;
    ep->qframes = 0;
    memset(&seg, 0, sizeof(seg));
    for (f = 0; f < n_frames; ++f) {
        int speech_count;
        ep_push(ep, is_speech[f]);
        ep->timestamp += ep->frame_length;
        speech_count = ep_speech_count(ep);
        if (ep->in_speech) {
            if (speech_count < ep->end_frames) {
                if (ep_pop(ep, NULL))
                    seg.n_samples += ep->frame_size;
                ep->speech_end = ep->qstart_time;
                ep->in_speech = 0;
                seg.speech_start = ep->speech_start;
                seg.speech_end = ep->speech_end;
                if (seg_push(out, &seg) < 0)
                    return -1;
                continue;
            }
        } else if (speech_count > ep->start_frames) {
            ep->speech_start = ep->qstart_time;
            ep->speech_end = 0;
            ep->in_speech = 1;
            seg.first_sample = ep->qframes * ep->frame_size;
            seg.n_samples = 0;
        }
        if (ep->in_speech && ep_pop(ep, NULL))
            seg.n_samples += ep->frame_size;
    }
    if (ep->in_speech) {
        int64_t out_nsamp = 0;
        ep->in_speech = 0;
        ep->speech_end = ep->qstart_time;
        ep_linearize(ep, tmp);
        while (ep->n != 0) {
            int is = 0;
            ep_pop(ep, &is);
            if (!is)
                break;
            out_nsamp += ep->frame_size;
            ep->speech_end = ep->qstart_time;
        }
        if (ep->n == 0 && ep->speech_end == ep->qstart_time) {
            ep->timestamp += (double)tail / ep->sample_rate;
            out_nsamp += tail;
            ep->speech_end = ep->timestamp;
        }
        seg.n_samples += out_nsamp;
        seg.speech_start = ep->speech_start;
        seg.speech_end = ep->speech_end;
        if (seg_push(out, &seg) < 0)
            return -1;
    }
    return 0;
}

ssw_endpoints_t *
ssw_endpoints_replay(const ssw_vad_t *v, double window, double ratio, const int8_t *is_speech,
                     const int32_t *frame_off, const int64_t *tail, int32_t n_streams)
{
    ep_t ep;
    seg_list_t list = { NULL, 0, 0 };
    ssw_endpoints_t *e = NULL;
    int8_t *tmp = NULL;
    int32_t u;
    if (v == NULL || n_streams < 0 || frame_off == NULL || tail == NULL
        || (frame_off[n_streams] > 0 && is_speech == NULL)) {
        ssw_set_error("endpointer: bad arguments");
        return NULL;
    }
    if (ep_configure(v, window, ratio, &ep) < 0)
        return NULL;
    for (u = 0; u < n_streams; ++u)
        if (tail[u] < 0 || tail[u] > v->frame_size) {
            ssw_set_error("Final frame must be %d samples or less", v->frame_size);
            return NULL;
        }
    ep.is = (int8_t *)malloc((size_t)ep.maxlen);
    tmp = (int8_t *)malloc((size_t)ep.maxlen);
    e = (ssw_endpoints_t *)calloc(1, sizeof(*e));
    if (e != NULL)
        e->seg_off = (int32_t *)calloc((size_t)n_streams + 1, sizeof(int32_t));
    if (ep.is == NULL || tmp == NULL || e == NULL || e->seg_off == NULL)
        goto no_memory;
    e->n_streams = n_streams;
    for (u = 0; u < n_streams; ++u) {
        if (ep_replay(&ep, is_speech + frame_off[u], frame_off[u + 1] - frame_off[u], tail[u], tmp,
                      &list) < 0)
            goto no_memory;
        e->seg_off[u + 1] = list.n;
    }
    e->segs = list.segs;
    free(ep.is);
    free(tmp);
    return e;
no_memory:
    ssw_set_error("endpointer: out of memory");
    free(ep.is);
    free(tmp);
    free(list.segs);
    if (e != NULL)
        free(e->seg_off);
    free(e);
    return NULL;
}

ssw_endpoints_t *
ssw_endpoints_from_decisions(const ssw_vad_t *v, double window, double ratio,
                             const int8_t *is_speech, int64_t n_frames, int64_t tail_samples)
{
    int32_t frame_off[2];
    if (n_frames < 0 || n_frames > INT32_MAX) {
        ssw_set_error("endpointer: bad arguments");
        return NULL;
    }
    frame_off[0] = 0;
    frame_off[1] = (int32_t)n_frames;
    return ssw_endpoints_replay(v, window, ratio, is_speech, frame_off, &tail_samples, 1);
}

int32_t ssw_endpoints_streams(const ssw_endpoints_t *e) { return e ? e->n_streams : -1; }

int32_t
ssw_endpoints_count(const ssw_endpoints_t *e, int32_t stream)
{
    if (e == NULL || stream < 0 || stream >= e->n_streams)
        return -1;
    return e->seg_off[stream + 1] - e->seg_off[stream];
}

int
ssw_endpoints_get(const ssw_endpoints_t *e, int32_t stream, int32_t k, ssw_endpoint_seg_t *out)
{
    const int32_t n = ssw_endpoints_count(e, stream);
    if (n < 0 || k < 0 || k >= n || out == NULL) {
        ssw_set_error("ssw_endpoints_get: no such segment");
        return -1;
    }
    *out = e->segs[e->seg_off[stream] + k];
    return 0;
}

void
ssw_endpoints_free(ssw_endpoints_t *e)
{
    if (e == NULL)
        return;
    free(e->seg_off);
    free(e->segs);
    free(e);
}
