/* ssw_k13_vad.inc -- vad_batch_kernel: vad_classify (src/ps_vad.c:154-160) over every whole frame
 * of a batch of streams.  The arithmetic is ssw_vad_core.inc, the source the host path is built
 * from; this file is the assignment of streams to lanes and the movement of data.
 *
 * A lane per stream, one wave per workgroup, `spw` (streams per workgroup, <= 64) of its lanes in
 * use.  A stream's frames are strictly sequential and all of the detector's state is per stream,
 * so nothing crosses lanes but the staging of audio.
 *
 * Everything a lane indexes with a run-time index lives in LDS, not in private arrays (which
 * would be scratch memory touched once per sample): the stream's ssw_vad_state_t, the frame at
 * 8 kHz, the four band buffers of WebRtcVad_CalculateFeatures and the features, VW_SLOTS int16
 * slots per stream.  Slot i of lane l is lds[i * SSW_VAD_PITCH + l] with a pitch of 66 int16 =
 * 33 dwords: the lanes of a wave reading one slot touch consecutive dwords, and one stream's
 * consecutive slots, written by the lanes of a wave when audio or state is staged, fall on
 * consecutive banks as well (33 = 1 mod 32).
 *
 * Audio is staged through LDS a chunk of VAD_CHUNK samples at a time: for each stream of the
 * workgroup in turn the wave loads the chunk with consecutive lanes on consecutive samples, then
 * every lane consumes its own stream's chunk through the resampler into the 8 kHz frame.  A
 * chunk is a multiple of 12 samples, the resamplers' largest group, and so are the frame sizes
 * at 48 kHz; at the other rates a frame's last chunk is shorter and still a multiple of 4.
 *
 * Ragged batches: the frame loop runs to the longest stream of the workgroup, the same count for
 * every lane, and a lane past its stream's end skips the work between the barriers. */
#define VAD_FN __device__ __forceinline__
#define SSW_VAD_PITCH 66
#define VAD_UNROLL _Pragma("unroll")
#define VAD_NOUNROLL _Pragma("clang loop unroll(disable) vectorize(disable)")
#include "ssw_vad_core.inc"

enum { VAD_CHUNK = 96, VAD_LANES = 64 };

struct VadParams {
    const int16_t *pcm;
    const int64_t *samp_off;  /* [n_streams + 1] */
    const int32_t *frame_off; /* [n_streams + 1] */
    int8_t *is_speech;        /* [total frames] */
    int16_t *feat;            /* [total frames][7] */
    ssw_vad_state_t *state;   /* [n_streams], read unless fresh, written */
    int32_t n_streams, spw, fresh;
    int32_t frame_size, nb_len;
    vad_thresholds_t th;
};

static size_t
vad_lds_bytes()
{
    return sizeof(int16_t) * (size_t)SSW_VAD_PITCH * (VW_SLOTS + VAD_CHUNK);
}

/* RATE: the detector's rate, a compile-time constant so that each instantiation holds one
 * resampler's constants (all four in one kernel spilt scalar registers) */
template <int RATE>
__global__ void __launch_bounds__(VAD_LANES)
vad_batch_kernel(const VadParams P)
{
    extern __shared__ int16_t vad_lds[];
    __shared__ int64_t s_base[VAD_LANES];
    __shared__ int32_t s_nfr[VAD_LANES];
    const int lane = threadIdx.x;
    const int u = blockIdx.x * P.spw + lane;
    const bool mine = lane < P.spw && u < P.n_streams;
    int16_t *const w = vad_lds + lane;
    int16_t *const stage = vad_lds + (size_t)SSW_VAD_PITCH * VW_SLOTS;
    const int32_t row0 = mine ? P.frame_off[u] : 0;
    const int32_t my_frames = mine ? P.frame_off[u + 1] - row0 : 0;
    s_base[lane] = mine ? P.samp_off[u] : 0;
    s_nfr[lane] = my_frames;
    /* the streams' states, a stream at a time with the lanes along its slots */
    if (!P.fresh) {
        VAD_NOUNROLL
        for (int s = 0; s < P.spw; ++s) {
            const int us = blockIdx.x * P.spw + s;
            if (us >= P.n_streams)
                break;
            const int16_t *src = (const int16_t *)(P.state + us);
            VAD_NOUNROLL
            for (int k = lane; k < VAD_STATE_SLOTS; k += VAD_LANES)
                vad_lds[k * SSW_VAD_PITCH + s] = src[k];
        }
    }
    __syncthreads();
    if (mine && (P.fresh || VW(w, VOFF(initialised)) != 42))
        vad_core_init(w);
    int max_frames = 0;
    VAD_NOUNROLL
    for (int s = 0; s < P.spw; ++s)
        max_frames = max(max_frames, s_nfr[s]);
    max_frames = __builtin_amdgcn_readfirstlane(max_frames);

    /* WebRtcVad_CalcVad48khz (vad_core.c:607-630) hands the resampler the frame's START once per
     * 10 ms of frame: the first 480 samples go through it frame_size / 480 times, each pass
     * advancing the resampler's state and filling the next 80 samples of the 8 kHz frame */
    const int n_in = RATE == 48000 ? 480 : P.frame_size;
    const int reps = RATE == 48000 ? P.frame_size / 480 : 1;
    VAD_NOUNROLL
    for (int f = 0; f < max_frames; ++f) {
        const bool act = f < my_frames;
        int nb_pos = 0;
        VAD_NOUNROLL
        for (int rep = 0; rep < reps; ++rep) {
            VAD_NOUNROLL
            for (int c0 = 0; c0 < n_in; c0 += VAD_CHUNK) {
                const int len = min((int)VAD_CHUNK, n_in - c0);
                VAD_NOUNROLL
                for (int s = 0; s < P.spw; ++s) {
                    const int nfr = __builtin_amdgcn_readfirstlane(s_nfr[s]);
                    if (f >= nfr)
                        continue;
                    const int64_t base = s_base[s]; /* (the same for every lane) */
                    const int16_t *src = P.pcm + base + (int64_t)f * P.frame_size + c0;
                    VAD_NOUNROLL
                    for (int j = lane; j < len; j += VAD_LANES)
                        stage[j * SSW_VAD_PITCH + s] = src[j];
                }
                __syncthreads();
                if (act)
                    nb_pos += vad_ingest(w, RATE, stage + lane, len, nb_pos);
                __syncthreads();
            }
        }
        if (act) {
            const int d = vad_decide(w, P.nb_len, P.th);
            const int64_t row = (int64_t)row0 + f;
            P.is_speech[row] = (int8_t)d;
            VAD_UNROLL
            for (int i = 0; i < 7; ++i)
                P.feat[row * 7 + i] = VW(w, VW_FEAT + i);
        }
    }
    __syncthreads();
    /* the states back, as they came */
    VAD_NOUNROLL
    for (int s = 0; s < P.spw; ++s) {
        const int us = blockIdx.x * P.spw + s;
        if (us >= P.n_streams)
            break;
        int16_t *dst = (int16_t *)(P.state + us);
        VAD_NOUNROLL
        for (int k = lane; k < VAD_STATE_SLOTS; k += VAD_LANES)
            dst[k] = vad_lds[k * SSW_VAD_PITCH + s];
    }
}
#undef VAD_FN
#undef VAD_UNROLL
#undef VAD_NOUNROLL
