/* ssw_slot_layout.inc -- host: the order in which the senone kernels visit the senones, and the
 * shape of their workgroups.  Plain C++17, no HIP header: ssw_kernels.hip includes it ahead of
 * the ssw_host_*.inc files, and a host program can include it on its own
 * (tests/harness/slot_layout_host.cpp). */
#include <cstddef>
#include <cstdint>
#include <vector>

/* Slots are grouped by codebook, ascending senone id inside a group, four slots (a quad) per
 * lane of ptm_senone_kernel.
 *   dense:  a group's ids side by side, the group's END padded to a multiple of 4.  A quad may
 *           then straddle two runs of consecutive ids (0 1 2 | 137), which only a store per
 *           slot can write out.
 *   prefix: a group's ids cut into maximal runs of consecutive ids, EVERY RUN's end padded to a
 *           multiple of 4.  Every quad then holds n = 1..4 consecutive ids s0 .. s0 + n - 1 in
 *           its first n slots and padding (-1) behind them: an 8-, a 4- and a 2-byte store write
 *           it out, no quad mixes two runs.
 * quad_n[q] = that n wherever a quad has this form, in either layout; 0 = it has not (the
 * kernels' store per slot).  quad_s0[q] = the quad's first slot's senone (always one). */
struct SlotLayout {
    std::vector<int16_t> slot_sen; /* [4 * n_quads] senone of every slot, -1 = padding */
    std::vector<uint8_t> quad_cb;  /* [n_quads] */
    std::vector<int16_t> quad_s0;  /* [n_quads] */
    std::vector<uint8_t> quad_n;   /* [n_quads] */
};

static inline SlotLayout
slot_layout(const int16_t *sen2cb, int n_sen, int n_cb, bool prefix)
{
    SlotLayout L;
    for (int c = 0; c < n_cb; ++c) {
        const size_t start = L.slot_sen.size();
        int prev = -2;
        for (int i = 0; i < n_sen; ++i) {
            if (sen2cb[i] != c)
                continue;
            if (prefix && i != prev + 1) /* a new run: close the last one's quad */
                while (L.slot_sen.size() % 4)
                    L.slot_sen.push_back(-1);
            L.slot_sen.push_back((int16_t)i);
            prev = i;
        }
        while (L.slot_sen.size() % 4)
            L.slot_sen.push_back(-1);
        for (size_t q = start / 4; q < L.slot_sen.size() / 4; ++q)
            L.quad_cb.push_back((uint8_t)c);
    }
    const size_t n_quads = L.quad_cb.size();
    L.quad_s0.resize(n_quads);
    L.quad_n.resize(n_quads);
    for (size_t q = 0; q < n_quads; ++q) {
        const int16_t *sj = &L.slot_sen[4 * q];
        int n = 1;
        while (n < 4 && sj[n] == sj[0] + n)
            ++n;
        bool form = true; /* ... and nothing but padding behind them */
        for (int j = n; j < 4; ++j)
            form = form && sj[j] < 0;
        L.quad_s0[q] = sj[0];
        L.quad_n[q] = (uint8_t)(form ? n : 0);
    }
    return L;
}

/* Shape of the batch senone kernels' workgroups for a model of n_quads quads, fpb frames per
 * group (launch_senone, ssw_host_score.inc, where the measurements behind it are written down):
 * R quads per thread, `threads` a multiple of 64 and at least 256.  seven_waves: the kernel is
 * ptm_senone_kernel, which prefers groups of about seven waves at two frames per group.
 * force_r: SSW_SEN_R, 0 = none.  The caller checks threads against its limits. */
struct SenoneShape {
    int R, threads;
};

static inline SenoneShape
senone_shape(int n_quads, int fpb, bool seven_waves, int force_r, int max_threads)
{
    SenoneShape s;
    s.R = (n_quads + max_threads - 1) / max_threads;
    if (seven_waves && fpb == 2 && s.R < 4) {
        const int r7 = (n_quads + 447) / 448;
        s.R = r7 > s.R ? (r7 > 4 ? 4 : r7) : s.R;
    }
    if (force_r != 0)
        s.R = force_r;
    if (s.R < 1)
        s.R = 1;
    s.threads = ((n_quads + s.R - 1) / s.R + 63) & ~63;
    if (s.threads < 256)
        s.threads = 256;
    return s;
}

/* The prefix layout is worth its extra quads (at most one per run) only while a thread's chain
 * work stays what it was: it is used if it needs no larger R and no more threads per group than
 * the dense layout, at one and at two frames per group, with and without the seven-wave rule.
 * A model of scattered ids (every id a run of its own) would multiply its slots: it keeps the
 * dense layout and the store per slot. */
static inline bool
slot_layout_prefix_fits(int dense_quads, int prefix_quads, int max_threads)
{
    for (int fpb = 1; fpb <= 2; ++fpb)
        for (int seven = 0; seven < 2; ++seven) {
            const SenoneShape d = senone_shape(dense_quads, fpb, seven != 0, 0, max_threads);
            const SenoneShape p = senone_shape(prefix_quads, fpb, seven != 0, 0, max_threads);
            if (p.R > d.R || p.threads > d.threads)
                return false;
        }
    return true;
}
