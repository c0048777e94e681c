/* ssw_active_set.inc -- host, no HIP: the active set of the reference's second pass
 * (state_align_search over acmod's growing bit vector) as a function of the phone windows alone:
 * active_first_frames, ActiveSetBuilder, and cont_active_rows, which turns them into the bitmap
 * rows cont_listed_kernel reads.  ssw_kernels.hip includes it ahead of ssw_host_active.inc; a host
 * program can include it on its own (tests/harness/cont_listed_host.cpp), with ssw_internal.h,
 * <algorithm>, <climits>, <cstdint> and <vector> before it. */

/* Which phones of an utterance are active in which frames.  state_align_search has no beam:
 * phone 0 is entered at frame 0; a phone active in frame t stays active in t + 1 unless
 * t + 1 > ef[i] (prune_hmms); phone i + 1 is entered in frame t + 1 as soon as phone i is active
 * there and t + 1 >= sf[i + 1] (phone_transition; "if inactive" enters whatever the score).  With
 * windows that do not decrease along the phones (what alignment_populate produces: the phones of
 * a word share their word's window) none of this depends on a score:
 *     first[0] = 0,  first[i] = max(1, sf[i], first[i - 1]),  active = [first[i], ef[i]],
 * and a phone whose first frame lies beyond its predecessor's last is never entered (nor any
 * after it).  acmod's active bit vector is never cleared by this search
 * (src/state_align_search.c:186-189; acmod_clear_active is only called by fsg_search), so the
 * set of frame t is the seed plus the senones of every phone with first[i] <= t. */
static int
active_first_frames(const int32_t *sf, const int32_t *ef, int n_phones, int n_frames,
                    std::vector<int32_t> &first)
{
    first.assign((size_t)n_phones, INT_MAX);
    int32_t prev_first = 0, prev_last = 0;
    for (int i = 0; i < n_phones; ++i) {
        if (i > 0 && (sf[i] < sf[i - 1] || ef[i] < ef[i - 1])) {
            ssw_set_error("ssw_align_batch_active: phone windows must not decrease along an "
                          "utterance (phone %d); with such windows the reference's active set "
                          "depends on the path scores", i);
            return -1;
        }
        int32_t fi = i == 0 ? 0 : std::max(std::max((int32_t)1, sf[i]), prev_first);
        if (i > 0 && fi > prev_last)
            break; /* never entered: the alignment fails, nothing more becomes active */
        if (fi >= n_frames)
            break;
        first[i] = fi;
        prev_first = fi;
        prev_last = ef[i] < fi ? fi : ef[i]; /* entered at fi it is active in fi at least */
    }
    return 0;
}

/* The listed senones of an utterance as the search's set grows (the header of
 * senone_active2_kernel, ssw_k1b_senone.inc): REAL senones in the order they are first listed,
 * and the bridge entries acmod_flags2list inserts where two listed neighbours are more than 255
 * apart (src/acmod.c:966-975; the scorer decodes them as listed senones, src/ptm_mgau.c:342-352),
 * kept up to date under insertions -- a new senone only changes the bridges of the one gap it
 * falls into.  The set is a bit per senone (neighbours by word scans), the bridges a short
 * sorted vector: no allocation per insertion (a node-based set made the host side of a
 * 256-utterance call 10 ms). */
struct ActiveSetBuilder {
    std::vector<uint64_t> bits;
    std::vector<int> bridges; /* ascending */
    std::vector<int> order;   /* real senones by first listing */
    explicit ActiveSetBuilder(int n_sen) : bits(((size_t)n_sen + 63) / 64, 0ull) {}
    int pred(int s) const /* largest listed senone below s, -1 if none */
    {
        int w = s >> 6;
        uint64_t v = bits[(size_t)w] & ((1ull << (s & 63)) - 1ull);
        for (;;) {
            if (v != 0ull)
                return w * 64 + 63 - __builtin_clzll(v);
            if (--w < 0)
                return -1;
            v = bits[(size_t)w];
        }
    }
    int succ(int s) const /* smallest listed senone above s, -1 if none */
    {
        int w = s >> 6;
        uint64_t v = (s & 63) == 63 ? 0ull : bits[(size_t)w] & ~((2ull << (s & 63)) - 1ull);
        for (;;) {
            if (v != 0ull)
                return w * 64 + __builtin_ctzll(v);
            if (++w >= (int)bits.size())
                return -1;
            v = bits[(size_t)w];
        }
    }
    /* bridges of the gap between listed neighbours lo < hi (lo = -1: the list's start, from
     * which the delta list counts as from senone 0) */
    void gap(int lo, int hi, bool add)
    {
        int last = lo < 0 ? 0 : lo;
        while (hi - last > 255) {
            last += 255;
            auto it = std::lower_bound(bridges.begin(), bridges.end(), last);
            if (add)
                bridges.insert(it, last);
            else if (it != bridges.end() && *it == last)
                bridges.erase(it);
        }
    }
    void insert(int s)
    {
        if ((bits[(size_t)s >> 6] >> (s & 63)) & 1ull)
            return;
        const int hi = succ(s), lo = pred(s);
        if (hi >= 0) {
            gap(lo, hi, false);
            gap(s, hi, true);
        }
        gap(lo, s, true);
        bits[(size_t)s >> 6] |= 1ull << (s & 63);
        order.push_back(s);
    }
};

/* One utterance of ssw_align_batch_active on a continuous model: every segment (a run of frames
 * that share their active set) as ONE bitmap row of nw32 = (n_sen + 31) / 32 words -- the seed,
 * the senones of every phone entered so far, and the bridges acmod_flags2list lists between them,
 * all ordinary bits -- appended to `rows`, and row_of_frame[t] = row_base + the segment of frame
 * t, for the utterance's n_frames frames.  senid: [n_phones][3]; seed: NULL or [nw32].
 * -1 with the message set: a senone out of range, windows that decrease (active_first_frames). */
static int
cont_active_rows(int n_sen, int n_frames, int n_phones, const uint16_t *senid, const int32_t *sf,
                 const int32_t *ef, const uint32_t *seed, int32_t row_base,
                 std::vector<uint32_t> &rows, int32_t *row_of_frame)
{
    const int nw32 = (n_sen + 31) / 32;
    if (n_frames < 0 || n_phones < 1) {
        ssw_set_error("ssw_align_batch_active: an utterance of %d phones, %d frames", n_phones, n_frames);
        return -1;
    }
    for (int p = 0; p < 3 * n_phones; ++p)
        if (senid[p] >= n_sen) {
            ssw_set_error("ssw_align_batch_active: phone %d: senone %d of %d", p / 3, senid[p], n_sen);
            return -1;
        }
    std::vector<int32_t> first;
    if (active_first_frames(sf, ef, n_phones, n_frames, first) < 0)
        return -1;
    ActiveSetBuilder B(n_sen);
    if (seed != NULL) /* what the first pass left active, ascending */
        for (int wd = 0; wd < nw32; ++wd) {
            uint32_t bits = seed[wd];
            while (bits) {
                const int sen = wd * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                if (sen < n_sen)
                    B.insert(sen);
            }
        }
    int next_phone = 0;
    int32_t row = row_base;
    for (int t = 0; t < n_frames; ++row) {
        /* phones entered by frame t join the set; the set then holds until the next entry */
        while (next_phone < n_phones && first[(size_t)next_phone] <= t) {
            for (int j = 0; j < 3; ++j)
                B.insert(senid[(size_t)next_phone * 3 + j]);
            ++next_phone;
        }
        const int t_end = next_phone < n_phones && first[(size_t)next_phone] < n_frames
            ? first[(size_t)next_phone] : n_frames;
        const size_t at = rows.size();
        rows.resize(at + (size_t)nw32, 0u);
        for (int wd = 0; wd < nw32; ++wd)
            rows[at + (size_t)wd] = (uint32_t)(B.bits[(size_t)wd >> 1] >> (32 * (wd & 1)));
        for (int b : B.bridges)
            rows[at + (size_t)(b >> 5)] |= 1u << (b & 31);
        for (; t < t_end; ++t)
            row_of_frame[t] = row;
    }
    return 0;
}
