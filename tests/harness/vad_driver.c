/* vad_driver.c -- the reference's own voice activity detector and endpointer, through its public
 * vad.h and endpointer.h only, for tests/golden/make_vad.py (linked against the reference library
 * that build() makes in oracle/_ref/) and tools/bench_vad.py.
 *
 *   vad_driver vad MODE RATE FRAMELEN PCM OUT
 *       vad_classify over every whole frame of PCM (raw int16); the classes as int8 to OUT;
 *       prints "frames frame_size sample_rate frame_length" (the length to 17 digits)
 *   vad_driver ep WINDOW RATIO MODE RATE FRAMELEN PCM
 *       endpointer_process over every whole frame, then endpointer_end_stream with the samples
 *       left over; prints one line per segment: "first_sample n_samples speech_start speech_end"
 *       (times to 17 digits).  first_sample is found from speech_start: the reference makes that
 *       time by adding the frame length once per frame that left the queue's head, so the same
 *       additions, counted, give the frame the segment starts with.
 *   vad_driver refuse-vad MODE RATE FRAMELEN | refuse-ep WINDOW RATIO MODE RATE FRAMELEN
 *       the init must return NULL; what the library reports goes to stderr as it comes
 *   vad_driver time MODE RATE FRAMELEN PCM REPS
 *       seconds of one pass of vad_classify over PCM, the best of REPS, on this core
 *
 * Exits 0, or 1 saying what failed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <soundswallower/endpointer.h>
#include <soundswallower/vad.h>

static void
die(const char *what)
{
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
}

static short *
read_pcm(const char *path, long *n)
{
    FILE *fh = fopen(path, "rb");
    short *pcm;
    long bytes;
    if (fh == NULL)
        die("cannot open the audio");
    fseek(fh, 0, SEEK_END);
    bytes = ftell(fh);
    fseek(fh, 0, SEEK_SET);
    pcm = malloc(bytes > 0 ? (size_t)bytes : 1);
    if (pcm == NULL || (bytes > 0 && fread(pcm, 1, (size_t)bytes, fh) != (size_t)bytes))
        die("cannot read the audio");
    fclose(fh);
    *n = bytes / 2;
    return pcm;
}

int
main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "vad")) {
        vad_t *vad = vad_init((vad_mode_t)atoi(argv[2]), atoi(argv[3]), strtod(argv[4], NULL));
        long n, f, frames;
        short *pcm = read_pcm(argv[5], &n);
        size_t size;
        signed char *out;
        FILE *fh;
        if (vad == NULL)
            die("vad_init refused");
        size = vad_frame_size(vad);
        frames = n / (long)size;
        out = malloc(frames > 0 ? (size_t)frames : 1);
        for (f = 0; f < frames; ++f)
            out[f] = (signed char)vad_classify(vad, pcm + f * (long)size);
        fh = fopen(argv[6], "wb");
        if (fh == NULL || fwrite(out, 1, (size_t)frames, fh) != (size_t)frames)
            die("cannot write the classes");
        fclose(fh);
        printf("%ld %ld %d %.17g\n", frames, (long)size, vad_sample_rate(vad), vad_frame_length(vad));
        vad_free(vad);
        free(out);
        free(pcm);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "ep")) {
        endpointer_t *ep = endpointer_init(strtod(argv[2], NULL), strtod(argv[3], NULL),
                                           (vad_mode_t)atoi(argv[4]), atoi(argv[5]),
                                           strtod(argv[6], NULL));
        long n, f, frames, first = 0, count = 0, k = 0;
        short *pcm = read_pcm(argv[7], &n);
        size_t size, out_nsamp = 0;
        double fl, acc = 0.0;
        int prev = 0;
        if (ep == NULL)
            die("endpointer_init refused");
        size = endpointer_frame_size(ep);
        fl = endpointer_frame_length(ep);
        frames = n / (long)size;
        for (f = 0; f < frames; ++f) {
            const short *got = endpointer_process(ep, pcm + f * (long)size);
            const int in = endpointer_in_speech(ep);
            if (!prev && in) {
                const double start = endpointer_speech_start(ep);
                while (acc != start) {
                    if (k > frames)
                        die("speech_start is not a sum of frame lengths");
                    acc += fl;
                    ++k;
                }
                first = k * (long)size;
                count = 0;
            }
            if (got != NULL)
                count += (long)size;
            if (prev && !in)
                printf("%ld %ld %.17g %.17g\n", first, count, endpointer_speech_start(ep),
                       endpointer_speech_end(ep));
            prev = in;
        }
        endpointer_end_stream(ep, pcm + frames * (long)size, (size_t)(n - frames * (long)size),
                              &out_nsamp);
        if (prev)
            printf("%ld %ld %.17g %.17g\n", first, count + (long)out_nsamp,
                   endpointer_speech_start(ep), endpointer_speech_end(ep));
        endpointer_free(ep);
        free(pcm);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "refuse-vad")) {
        if (vad_init((vad_mode_t)atoi(argv[2]), atoi(argv[3]), strtod(argv[4], NULL)) != NULL)
            die("vad_init accepted");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "refuse-ep")) {
        if (endpointer_init(strtod(argv[2], NULL), strtod(argv[3], NULL), (vad_mode_t)atoi(argv[4]),
                            atoi(argv[5]), strtod(argv[6], NULL)) != NULL)
            die("endpointer_init accepted");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "time")) {
        long n, f, frames;
        short *pcm = read_pcm(argv[5], &n);
        const int reps = atoi(argv[6]);
        double best = 1e30;
        long speech = 0;
        int r;
        for (r = 0; r < reps; ++r) {
            vad_t *vad = vad_init((vad_mode_t)atoi(argv[2]), atoi(argv[3]), strtod(argv[4], NULL));
            struct timespec t0, t1;
            size_t size;
            double s;
            if (vad == NULL)
                die("vad_init refused");
            size = vad_frame_size(vad);
            frames = n / (long)size;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            for (f = 0; f < frames; ++f)
                speech += vad_classify(vad, pcm + f * (long)size);
            clock_gettime(CLOCK_MONOTONIC, &t1);
            s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
            if (s < best)
                best = s;
            vad_free(vad);
        }
        printf("%.9f %ld\n", best, speech);
        free(pcm);
        return 0;
    }
    fprintf(stderr, "usage: vad_driver vad MODE RATE FRAMELEN PCM OUT | ep WINDOW RATIO MODE RATE "
                    "FRAMELEN PCM | refuse-vad MODE RATE FRAMELEN | refuse-ep WINDOW RATIO MODE "
                    "RATE FRAMELEN | time MODE RATE FRAMELEN PCM REPS\n");
    return 1;
}
