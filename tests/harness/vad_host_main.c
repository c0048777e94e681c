/* vad_host_main.c -- the host path of voice activity detection and endpointing (csrc/ssw_vad.c
 * over csrc/ssw_vad_core.inc: ssw_vad_create, ssw_vad_batch_host, ssw_endpoints_from_decisions) as
 * a stand-alone program, for tests/test_vad_host_sanitizers.py to run under AddressSanitizer +
 * UBSan.  The arithmetic is the kernel's, so what is clean here is the kernel's arithmetic too.
 *
 *   vad_host_main RATE PCM...
 *
 * Every PCM file (raw int16 at RATE Hz) goes through modes 0..3 x frame lengths 10, 20, 30 ms:
 * whole, then in two calls through `state` beside an empty stream, whose decisions and features
 * must be the whole stream's; the decisions are replayed through the endpointer at
 * (0.3, 0.9) and (0.5, 0.8) with every tail from 0 to 2 and size - 1.  The refusals are tried too.
 * Prints "ok N runs, S segments"; exits 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssw_internal.h"

static void
die(const char *what, const char *arg)
{
    fprintf(stderr, "FAILED: %s (%s): %s\n", what, arg, ssw_last_error());
    exit(1);
}

static void
must_refuse(int ok, const char *words)
{
    if (ok)
        die("accepted", words);
    if (strstr(ssw_last_error(), words) == NULL)
        die("refused in other words", words);
}

int
main(int argc, char **argv)
{
    static const double lengths[3] = { 0.01, 0.02, 0.03 };
    static const double windows[2][2] = { { 0.3, 0.9 }, { 0.5, 0.8 } };
    long n_runs = 0, n_segs = 0;
    int a, rate;
    if (argc < 3) {
        fprintf(stderr, "usage: vad_host_main RATE PCM...\n");
        return 1;
    }
    rate = atoi(argv[1]);
    must_refuse(ssw_vad_create(4, 16000, 0.03) != NULL, "Invalid VAD mode 4");
    must_refuse(ssw_vad_create(0, 100000, 0.03) != NULL, "No suitable sampling rate found for 100000");
    must_refuse(ssw_vad_create(0, 16000, 0.015) != NULL, "Unsupported frame length 0.015000");
    for (a = 2; a < argc; ++a) {
        FILE *fh = fopen(argv[a], "rb");
        long bytes, n;
        int16_t *pcm;
        int mode, li;
        if (fh == NULL)
            die("cannot open", argv[a]);
        fseek(fh, 0, SEEK_END);
        bytes = ftell(fh);
        fseek(fh, 0, SEEK_SET);
        n = bytes / 2;
        pcm = (int16_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(*pcm)); /* exactly n: a read past it shows */
        if (pcm == NULL || fread(pcm, sizeof(*pcm), (size_t)n, fh) != (size_t)n)
            die("cannot read", argv[a]);
        fclose(fh);
        for (mode = 0; mode < 4; ++mode) {
            for (li = 0; li < 3; ++li) {
                ssw_vad_t *v = ssw_vad_create(mode, rate, lengths[li]);
                int32_t size, frames, cut, fo[4], w, k;
                int64_t off[3];
                int8_t *whole, *pieces;
                int16_t *feat_whole, *feat_pieces;
                ssw_vad_state_t state[3];
                if (v == NULL)
                    die("ssw_vad_create", argv[a]);
                size = ssw_vad_frame_size(v);
                frames = (int32_t)ssw_vad_frame_count(v, n);
                whole = (int8_t *)malloc((size_t)frames + 1);
                pieces = (int8_t *)malloc(3 * (size_t)frames + 1);
                feat_whole = (int16_t *)malloc(sizeof(int16_t) * 7 * ((size_t)frames + 1));
                feat_pieces = (int16_t *)malloc(sizeof(int16_t) * 7 * (3 * (size_t)frames + 1));
                if (!whole || !pieces || !feat_whole || !feat_pieces)
                    die("out of memory", argv[a]);
                off[0] = 0;
                off[1] = n;
                if (ssw_vad_batch_host(v, pcm, off, 1, whole, fo, NULL, feat_whole) < 0 || fo[1] != frames)
                    die("ssw_vad_batch_host", argv[a]);
                /* a batch of two streams, the head and an empty one, then their rests through
                 * `state` (all zeros: not set up, so the first call starts afresh) */
                cut = frames / 2;
                memset(state, 0, sizeof(state));
                ssw_vad_state_init(&state[2]);
                off[0] = 0;
                off[1] = off[2] = (int64_t)cut * size;
                if (ssw_vad_batch_host(v, pcm, off, 2, pieces, fo, state, feat_pieces) < 0)
                    die("first piece", argv[a]);
                off[0] = (int64_t)cut * size;
                off[1] = off[2] = (int64_t)frames * size;
                if (ssw_vad_batch_host(v, pcm, off, 2, pieces + cut, fo, state, feat_pieces + 7 * cut) < 0)
                    die("second piece", argv[a]);
                if (memcmp(pieces, whole, (size_t)frames) != 0
                    || memcmp(feat_pieces, feat_whole, sizeof(int16_t) * 7 * (size_t)frames) != 0)
                    die("two pieces differ from the whole", argv[a]);
                off[0] = 0;
                off[1] = n;
                if (ssw_vad_batch_host(v, pcm, off, 1, pieces, fo, &state[2], NULL) < 0
                    || memcmp(pieces, whole, (size_t)frames) != 0)
                    die("an initialised state differs from none", argv[a]);
                for (w = 0; w < 2; ++w) {
                    static const int tails[4] = { 0, 1, 2, -1 };
                    for (k = 0; k < 4; ++k) {
                        const int64_t tail = tails[k] < 0 ? size - 1 : tails[k];
                        ssw_endpoints_t *e = ssw_endpoints_from_decisions(v, windows[w][0], windows[w][1],
                                                                           whole, frames, tail);
                        ssw_endpoint_seg_t seg;
                        int32_t s, count;
                        if (e == NULL)
                            die("ssw_endpoints_from_decisions", argv[a]);
                        count = ssw_endpoints_count(e, 0);
                        for (s = 0; s < count; ++s) {
                            if (ssw_endpoints_get(e, 0, s, &seg) < 0 || seg.first_sample < 0
                                || seg.n_samples < 0 || seg.first_sample + seg.n_samples > n + size
                                || !(seg.speech_end >= seg.speech_start))
                                die("a segment outside the stream", argv[a]);
                        }
                        n_segs += count;
                        ssw_endpoints_free(e);
                    }
                }
                must_refuse(ssw_endpoints_from_decisions(v, 0.3, 0.999, whole, frames, 0) != NULL,
                            "makes end-pointing stupid or impossible");
                must_refuse(ssw_endpoints_from_decisions(v, 0.3, 0.9, whole, frames, size + 1) != NULL,
                            "Final frame must be");
                free(whole);
                free(pieces);
                free(feat_whole);
                free(feat_pieces);
                ssw_vad_free(v);
                ++n_runs;
            }
        }
        free(pcm);
    }
    printf("ok %ld runs, %ld segments\n", n_runs, n_segs);
    return 0;
}
