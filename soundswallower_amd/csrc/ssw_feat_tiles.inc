/* ssw_feat_tiles.inc -- host: how ssw_feat_batch_ex cuts a batch into tiles.  Plain C++17, no
 * HIP header: ssw_kernels.hip includes it ahead of ssw_host_featex.inc, and a host program can
 * include it on its own (tests/harness/feat_tiles_host.cpp). */
#include <cstddef>
#include <cstdint>
#include <vector>

/* Frames per tile for a configuration of C cepstra, window W, R raw dimensions, J LDA rows
 * (0 = none) and a subvector gather or not: the most, up to 64, whose LDS image
 *   (tf + 2 W) C  normalised cepstra | tf R raw rows (with an LDA or a gather) | tf J (with both)
 * stays within lds_budget bytes; *lds_bytes is that image.  0 when not even one frame fits. */
static inline int
feat_tile_frames(int C, int W, int R, int J, bool gather, size_t lds_budget, size_t *lds_bytes)
{
    const size_t per_frame = (size_t)C + (J > 0 || gather ? (size_t)R : 0) + (J > 0 && gather ? (size_t)J : 0);
    const size_t fixed = (size_t)2 * W * C;
    const size_t floats = lds_budget / sizeof(float);
    if (floats < fixed + per_frame)
        return 0;
    size_t tf = (floats - fixed) / per_frame;
    if (tf > 64)
        tf = 64;
    *lds_bytes = (fixed + tf * per_frame) * sizeof(float);
    return (int)tf;
}

/* The tile table of a batch: pairs (utterance, first frame counted from the batch's frame 0),
 * utterance after utterance, tf frames each but an utterance's last, which holds the rest; an
 * empty utterance has none, and no tile spans two utterances.  Returns the number of tiles, or
 * -1 when utt_off does not run from 0 to n_frames without decreasing (nothing usable is left
 * in `tiles` then). */
static inline long
feat_tiles_build(const int32_t *utt_off, int32_t n_utts, int32_t n_frames, int32_t tf,
                 std::vector<int32_t> &tiles)
{
    tiles.clear();
    if (utt_off == nullptr || n_utts < 0 || n_frames < 0 || tf < 1 || utt_off[0] != 0
        || utt_off[n_utts] != n_frames)
        return -1;
    for (int32_t u = 0; u < n_utts; ++u)
        if (utt_off[u + 1] < utt_off[u])
            return -1;
    tiles.reserve(2 * ((size_t)n_frames / (size_t)tf + (size_t)n_utts));
    for (int32_t u = 0; u < n_utts; ++u)
        for (int64_t f = utt_off[u]; f < utt_off[u + 1]; f += tf) {
            tiles.push_back(u);
            tiles.push_back((int32_t)f);
        }
    return (long)(tiles.size() / 2);
}
