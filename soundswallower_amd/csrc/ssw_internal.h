/* ssw_internal.h -- shared between the host C loaders and the HIP translation unit. */
#ifndef SSW_INTERNAL_H
#define SSW_INTERNAL_H

#include "ssw_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSW_SENSCR_SHIFT 10
#define SSW_WORST_SCORE ((int32_t)0xE0000000)
#define SSW_MAX_NEG_ASCR 96
#define SSW_MAX_NEG_MIXW 159
#define SSW_MAX_FEAT 8

/* Gaussian record on the device: one density = 32 floats = one 128-byte line.
 *   [0 .. veclen)  mean      [15] det      [16 .. 16+veclen)  precomputed 1/(2 var) scale
 * Unused slots are 0.0f, which makes a padded dimension an exact no-op (d - 0*0*0 = d). */
#define SSW_REC_FLOATS 32
#define SSW_REC_DET 15
#define SSW_REC_VAR 16
#define SSW_MAX_VECLEN 15
/* per codebook-stream: [0] count, [1..] codewords the quadratic scan leaves to the exact form */
#define SSW_EXLIST_STRIDE 132
/* matrix-core scan: binary16 values per (codebook, stream) in wfrag */
#define SSW_WFRAG_PER_CBF (4 * 2 * 2 * 64 * 8)

/* s2_semi scorer (ssw_k10_semi.inc): one codebook, streams of up to 32 dimensions, up to 256
 * densities; its Gaussian table holds SSW_SC_ROWS rows of SSW_SC_MAX_DENSITY floats per stream */
#define SSW_SC_MAX_VECLEN 32
#define SSW_SC_MAX_DENSITY 256
#define SSW_SC_MAX_TOPN 4
#define SSW_SC_ROWS (2 * SSW_SC_MAX_VECLEN + 1)

/* continuous-density models (one codebook per senone, ssw_k11_cont.inc): streams of up to 64
 * dimensions, up to 64 densities, topn up to 8 or every density */
#define SSW_CONT_MAX_VECLEN 64
#define SSW_CONT_MAX_DENSITY 64
#define SSW_CONT_MAX_TOPN 8

/* MFCC front end (ssw_model.c, ssw_k8_fe.inc, ssw_host_fe.inc): ssw_fe_batch's one framing,
 * 16 kHz, 100 frames/s, 25.625 ms window, 512-point FFT; ssw_fe_batch_ex frames at any rate
 * with FFTs of SSW_FE_MIN_NFFT .. SSW_FE_MAX_NFFT points */
#define SSW_FE_FRAME 410
#define SSW_FE_SHIFT 160
#define SSW_FE_NFFT 512
#define SSW_FE_MIN_LOG2N 6
#define SSW_FE_MAX_LOG2N 13
#define SSW_FE_MIN_NFFT (1 << SSW_FE_MIN_LOG2N)
#define SSW_FE_MAX_NFFT (1 << SSW_FE_MAX_LOG2N)
#define SSW_FE_MAX_FILT 64
#define SSW_FE_NCEP 13

/* the part of the front end's tables that does not depend on the rate (ssw_fe_tables_build) */
typedef struct ssw_fe_tables_s {
    int32_t nfilt, ncep, transform, remove_noise, lifter_val;
    float alpha, sqrt_inv_n, sqrt_inv_2n;
    float mel_cosine[SSW_FE_NCEP * SSW_FE_MAX_FILT]; /* [ncep][nfilt] */
    float lifter[SSW_FE_NCEP];
} ssw_fe_tables_t;

/* one rate's framing, as fe_parse_general_params and fe_init derive it (ssw_fe_framing) */
typedef struct ssw_fe_framing_s {
    int32_t samprate, frame_shift, frame_size, fft_size, fft_order;
} ssw_fe_framing_t;

/* the part that depends on the rate, one variable-size block per (samprate, nfft)
 * (ssw_fe_rate_build): this header, then double hamming[frame_size / 2], double
 * ccc[fft_size / 4], double sss[fft_size / 4] and float filt_coeffs[n_coeffs] at the byte
 * offsets it records; `bytes` is the whole block */
typedef struct ssw_fe_rate_s {
    int32_t samprate, frame_shift, frame_size, fft_size, fft_order, nfilt, n_coeffs, bytes;
    int32_t hamming_off, ccc_off, sss_off, coeff_off;
    int32_t spec_start[SSW_FE_MAX_FILT], filt_width[SSW_FE_MAX_FILT], filt_start[SSW_FE_MAX_FILT];
} ssw_fe_rate_t;

/* feat_params.json over *c (which holds the defaults): 0 read, 1 no such file, -1 unusable
 * (message in err) */
int ssw_fe_config_read(const char *path, ssw_fe_config_t *c, char *err, size_t err_len);
/* the front end's string settings, which have no place in ssw_fe_config_t: "warp_type",
 * "warp_params" ("" when null or empty: no warping) and "input_endian" */
typedef struct ssw_fe_strings_s {
    char warp_type[32], warp_params[256], input_endian[16];
} ssw_fe_strings_t;
void ssw_fe_strings_defaults(ssw_fe_strings_t *s);
/* ssw_fe_config_read that keeps the strings too, over *s (which holds the defaults) */
int ssw_fe_config_read_strings(const char *path, ssw_fe_config_t *c, ssw_fe_strings_t *s,
                               char *err, size_t err_len);
/* 0 when ssw_fe_batch supports the configuration, else -1 and ssw_set_error */
int ssw_fe_config_check(const ssw_fe_config_t *c);
/* the same for ssw_fe_batch_ex: every setting but the rate and the framing, which
 * ssw_fe_framing checks per rate */
int ssw_fe_config_check_ex(const ssw_fe_config_t *c);
/* samprate (whole hertz; 0 = minimum_samprate of c->upperf) -> *f, or -1 and ssw_set_error */
int ssw_fe_framing(const ssw_fe_config_t *c, double samprate, ssw_fe_framing_t *f);
int ssw_fe_tables_build(const ssw_fe_config_t *c, ssw_fe_tables_t *t);
/* malloc'd block for c at framing f, or NULL and ssw_set_error (a filter that covers no DFT
 * point; with `finite`, one whose edges round onto one point, which makes NaN coefficients;
 * out of memory) */
ssw_fe_rate_t *ssw_fe_rate_build(const ssw_fe_config_t *c, const ssw_fe_framing_t *f, int finite);
int64_t ssw_fe_frames_of(int64_t n_samples);
int64_t ssw_fe_frames_at(const ssw_fe_framing_t *f, int64_t n_samples);

/* The front end in every configuration fe_init accepts (ssw_fe_create, ssw_fe_batch_any;
 * ssw_model.c, ssw_k8_fe_any.inc, ssw_host_fe_any.inc). */
#define SSW_FE_MAX_CEP 64
enum ssw_fe_warp { SSW_FE_WARP_INVERSE_LINEAR = 0, SSW_FE_WARP_AFFINE = 1,
                   SSW_FE_WARP_PIECEWISE_LINEAR = 2 }; /* FE_WARP_ID_*, fe_warp.c:68-73 */
enum ssw_fe_logspec { SSW_FE_CEPSTRA = 0, SSW_FE_RAW_LOG_SPEC = 1, SSW_FE_SMOOTH_LOG_SPEC = 2 };
/* how a frame's DC sum is formed: not at all, by a parallel reduction (the host proved that no
 * partial sum in any order rounds, ssw_fe_dc_sum_exact), or in index order */
enum ssw_fe_dc { SSW_FE_DC_NONE = 0, SSW_FE_DC_ANY_ORDER = 1, SSW_FE_DC_IN_ORDER = 2 };

/* a resolved configuration (ssw_fe_t): the settings, the warping function with its parameters as
 * the type's set_parameters parses them (the reference keeps them in statics), and what follows
 * from the settings alone */
struct ssw_fe_s {
    ssw_fe_config_t cfg;
    int32_t warp_id;     /* enum ssw_fe_warp */
    int32_t warp_on;     /* 0: is_neutral (no parameters, or slope 0) */
    float warp_p[2];     /* params[] */
    int32_t plain;       /* ssw_fe_batch_ex takes the settings: the existing kernels run */
    int32_t log_spec;    /* enum ssw_fe_logspec */
    int32_t out_dim;     /* fe_get_output_size */
    char warp_type[32], warp_params[256];
};

/* ssw_fe_tables_t for any ncep and every transform.  The first eight fields are ssw_fe_tables_t's:
 * fe_noise_kernel reads nfilt through that type */
typedef struct ssw_fe_any_tables_s {
    int32_t nfilt, ncep, transform, remove_noise, lifter_val;
    float alpha, sqrt_inv_n, sqrt_inv_2n;
    int32_t log_spec, remove_dc, out_dim, pad;
    float mel_cosine[SSW_FE_MAX_CEP * SSW_FE_MAX_FILT]; /* [ncep][nfilt] */
    float lifter[SSW_FE_MAX_CEP];
} ssw_fe_any_tables_t;

/* cfg with the warp strings (NULL type: inverse_linear; NULL or "" params: none) -> *fe, or -1
 * and ssw_set_error: everything ssw_fe_create refuses */
int ssw_fe_resolve(const ssw_fe_config_t *cfg, const char *warp_type, const char *warp_params,
                   struct ssw_fe_s *fe);
void ssw_fe_any_tables_build(const struct ssw_fe_s *fe, ssw_fe_any_tables_t *t);
/* ssw_fe_rate_build with fe's filter builder: doublebw, unit_area, round_filters and warping at
 * this rate's Nyquist frequency */
ssw_fe_rate_t *ssw_fe_any_rate_build(const struct ssw_fe_s *fe, const ssw_fe_framing_t *f);
/* 1 when every order of summing a frame of frame_size pre-emphasised int16 samples gives the
 * same double (f32 samples: never) */
int ssw_fe_dc_sum_exact(float alpha, int32_t frame_size, int f32);

/* Dynamic features (ssw_model.c, ssw_k12_feat.inc, ssw_host_featex.inc): a configuration as
 * feat_init_s3file resolves it (src/feat.c:732-927). */
#define SSW_FEAT_MAX_CEP 64
#define SSW_FEAT_MAX_WIN 8
#define SSW_FEAT_MAX_LDA_ROWS 256
/* one float of the raw feature vector (the streams back to back, before LDA and svspec) as the
 * reference's compute_feat functions form it (src/feat.c:437-712), packed into 32 bits:
 *   bits 0..1   op: 0  c[t+o0][i]                      (memcpy, feat_copy)
 *                   1  c[t+o0][i] - c[t+o1][i]          (a delta)
 *                   2  (c[t+o0][i] - c[t+o1][i]) - (c[t+o2][i] - c[t+o3][i])   (d1 - d2)
 *   bits 2..7   i, the cepstral dimension
 *   bits 8..27  o0..o3, each + SSW_FEAT_MAX_WIN in 5 bits */
#define SSW_FEAT_RECIPE(op, i, o0, o1, o2, o3)                                               \
    ((uint32_t)(op) | (uint32_t)(i) << 2 | (uint32_t)((o0) + SSW_FEAT_MAX_WIN) << 8           \
     | (uint32_t)((o1) + SSW_FEAT_MAX_WIN) << 13 | (uint32_t)((o2) + SSW_FEAT_MAX_WIN) << 18  \
     | (uint32_t)((o3) + SSW_FEAT_MAX_WIN) << 23)
typedef struct ssw_feat_plan_s {
    int32_t cepsize, window, n_stream, stream_len[SSW_MAX_FEAT], raw_dim;
    int32_t cmn, varnorm;      /* enum ssw_cmn */
    int32_t lda_rows;          /* rows used (feat->out_dim after feat_read_lda_s3file), 0 = no LDA */
    int32_t n_sv, sv_len[SSW_MAX_FEAT], sv_dim; /* svspec: subvectors, 0 = none */
    int32_t out_dim;           /* floats per output row: sv_dim, else lda_rows, else raw_dim */
    uint32_t *recipe;          /* [raw_dim] */
    float *lda_t;              /* [raw_dim][lda_rows]: matrix 0 of the file, transposed */
    int32_t *sv;               /* [sv_dim] dimensions gathered, in output order */
    float prior_mean[SSW_FEAT_MAX_CEP], prior_sum[SSW_FEAT_MAX_CEP]; /* cmn_set_repr(cmninit) */
    int32_t prior_nframe;
} ssw_feat_plan_t;
/* 0, or -1 and ssw_set_error; on success the caller owns the plan's arrays */
int ssw_feat_plan_build(const ssw_feat_config_t *c, ssw_feat_plan_t *p);
void ssw_feat_plan_free(ssw_feat_plan_t *p);
/* feat_params.json's FEAT_OPTIONS keys over *c: 0 read, 1 no such file, -1 unusable (err) */
int ssw_feat_config_read_err(const char *path, ssw_feat_config_t *c, char *err, size_t err_len);

/* Host-side model: every table derived exactly as the reference derives it. */
typedef struct ssw_host_model_s {
    ssw_config_t cfg;
    /* the feature stage's settings from the same feat_params.json, and why they could not be
     * read ("" when they could) */
    ssw_feat_config_t feat;
    char feat_err[256];
    /* front end: feat_params.json beside the means file (ssw_model.c); fe_err holds why that file
     * could not be used ("" when it could, or when there is none) */
    ssw_fe_config_t fe;
    ssw_fe_strings_t fe_str;
    char fe_err[256];
    /* Gaussians (gauden_t) */
    int32_t n_cb, n_feat, n_density, veclen_total, n_floored;
    int32_t veclen[SSW_MAX_FEAT], featoff[SSW_MAX_FEAT];
    float *mean, *var, *det; /* file order / [cb][feat][density] */
    /* the means and variances as the files hold them (un-precomputed), file order: what an MLLR
     * transform is applied to, and what its removal puts back (ssw_host_model_apply_mllr) */
    float *mean0, *var0;
    int32_t mllr_generation; /* 0 after load, +1 per transform applied or removed */
    /* device-layout Gaussian tables (ssw_host_build_records):
     *   rec     [cb*feat][density][32]  exact records (mean, det, scale)
     *   recq    [cb*feat][density][32]  quadratic-form scan records (a, c, b)
     *   recd0   [cb*feat][32]           [0] = the codebook's reference det d0; matrix-core
     *                                   scan: [1] = 2^s, [2] = 2^-s (its keys are key 2^-s),
     *                                   [3] = 2^ec (the constant's slot of X)
     *   exlist  [cb*feat][SSW_EXLIST_STRIDE] */
    float *rec, *recq, *recd0;
    uint32_t *exlist;
    int32_t n_exact_form;
    /* the same scan for the matrix cores (ssw_k1a_mfma.inc): quadratic-form records whose
     * constant carries the error bound of the split-binary16 MFMA evaluation (recqm, exlistm as
     * recq / exlist; recqm's constant is what its two parts add up to, unscaled), and the
     * records, scaled by 2^-s (the constant by 2^-(s + ec)), cut into two binary16 parts in MFMA
     * A-fragment order:
     *   wfrag [cb*feat][4 row blocks][2 K blocks][2 parts][64 lanes][8] binary16
     * (lane l of a fragment: density 32*rb + l%32, K = 16*kb + 8*(l/32) .. +7) */
    float *recqm;
    uint32_t *exlistm;
    uint16_t *wfrag;
    /* the exact records once more, packed for the matrix-core scan's LDS copy:
     * rec28 [cb*feat][density][28] = mean 0..12 | det 13 | scale 14..26 | 0 */
    float *rec28;
    int32_t n_exact_form_m;
    /* mdef */
    int32_t n_ciphone, n_phone, n_emit_state, n_ci_sen, n_sen, n_tmat, n_sseq, sil;
    uint16_t *sseq;
    int16_t *sen2cb; /* bin_mdef sen2cimap */
    int32_t *phone_ssid, *phone_tmat;
    /* context-dependent phone tree (cd_tree_t, bin_mdef.h:103-114), host byte order */
    int32_t n_cd_tree;
    struct ssw_cd_node_s { int16_t ctx, n_down; int32_t down_or_pid; } *cd_tree;
    char **ciname;       /* [n_ciphone] */
    uint8_t *ci_filler;  /* [n_ciphone] */
    /* tmat */
    uint8_t *tp;
    int32_t tp_n_tmat, tp_n_state;
    /* mixture weights */
    uint8_t *ptm_mixw; /* [feat][density][n_sen], 8-bit (4-bit clustered dumps are expanded) */
    uint8_t *ms_pdf;   /* [sen][feat][density] */
    /* log-add tables */
    uint8_t logadd8[256];
    /* memo of bin_mdef_phone_id_nearest, [pos][base][left][right], -2 = not looked up yet
     * (filled lazily by ssw_phone_id_nearest; racing writers store the same value) */
    int32_t *pid_memo;
    int32_t logadd8_size;   /* entries produced by logmath_init (>= 256) */
    int32_t zero8;          /* logmath zero at shift 10 */
    /* single-codebook models (the s2_semi scorer): sc_rec [n_feat][SSW_SC_ROWS]
     * [SSW_SC_MAX_DENSITY], see build_semi_records; NULL otherwise */
    float *sc_rec;
    /* continuous-density models (n_cb == n_sen, the ms scorer with sen2cb the identity): the
     * table of ssw_k11_cont.inc, see build_cont_records; NULL otherwise.  cont_sp = n_sen rounded
     * up to 64, cont_off[f] = floats before stream f's part, cont_floats = all of them */
    float *cont_rec;
    int32_t continuous, cont_sp;
    size_t cont_off[SSW_MAX_FEAT], cont_floats;
    /* the same floats senone-major, for cont_listed_kernel (ssw_host_build_cont_sm; NULL until
     * then): senone s owns cont_sm_sen floats, its stream f's record starts cont_sm_off[f] floats
     * in and holds, for n = n_density and v = veclen[f],
     *   [v][n][2]  (mean, scale) of dimension j, density d, as a pair
     *   [n]        det
     * padded with one 0.0f to an even count of floats */
    float *cont_rec_sm;
    size_t cont_sm_off[SSW_MAX_FEAT], cont_sm_sen, cont_sm_floats;
} ssw_host_model_t;

/* the scorer acmod_load_am would choose for the model's shape (enum ssw_scorer) */
int ssw_host_scorer(const ssw_host_model_t *h);

ssw_host_model_t *ssw_host_model_load(const char *mdef, const char *means,
                                      const char *variances, const char *sendump,
                                      const char *mixw, const char *tmat,
                                      const ssw_config_t *cfg);
void ssw_host_model_free(ssw_host_model_t *h);
int ssw_host_build_records(ssw_host_model_t *h);
/* Everything derived from (mean, raw variance): h->mean and h->var hold means and un-precomputed
 * variances in file order; the variances are floored and scaled in place, det is made, and the
 * tables of the model's scorer are rebuilt in the allocations they have (first call: made).  Both
 * the loader and ssw_host_model_apply_mllr end here. */
int ssw_host_derive_tables(ssw_host_model_t *h);
/* a continuous model's second table (cont_rec_sm above) from mean / var / det as they stand;
 * rebuilt in its allocation when it exists.  From then on ssw_host_derive_tables keeps it up to
 * date.  -1 and ssw_set_error: not a continuous model, out of memory (the model is unchanged). */
int ssw_host_build_cont_sm(ssw_host_model_t *h);
/* gauden_mllr_transform (src/ms_gauden.c:459-539) over the parameters as read: class 0 of the
 * transform on every codebook, then ssw_host_derive_tables.  NULL puts the files' parameters
 * back.  A transform that does not fit the model, or holds a non-finite number, is refused before
 * anything is touched: -1 and ssw_set_error. */
int ssw_host_model_apply_mllr(ssw_host_model_t *h, const ssw_mllr_t *mllr);
void ssw_set_error(const char *fmt, ...);

/* Pronunciation dictionary (ssw_lexicon.c) */
#define SSW_DICT_MAX_PRON 256 /* phones of one word: a dictionary line's are cut there */
struct ssw_dict_s {
    int n_words, cap_words;
    char **word;
    int16_t **pron; /* CI phone ids */
    int *pronlen;
    int *slot;      /* open-addressing hash: word index + 1, 0 = empty */
    int n_slots;
    int filler_start; /* first word that came from the filler dictionary (dict_filler_start) */
    int filler_end;   /* last word of the load, <s>, </s> and <sil> included (dict_filler_end,
                       * src/dict.c:337); fixed by ssw_dict_load, so words added later are past it */
    int *alt;        /* dict_nextalt: next alternate pronunciation of the same base word, -1 */
    int *base;        /* dict_basewid */
};
int ssw_dict_find(const struct ssw_dict_s *d, const char *w);

/* First-pass graphs of a batch of texts (ssw_fsg.c), flat arrays the kernel reads.
 * Node indices, leaf ordinals and states are local to their utterance. */
typedef struct ssw_fp_graphs_s {
    int32_t n_utts, n_nodes, n_leaves, n_states, n_in;
    int32_t *node_off, *leaf_off, *state_off; /* [n_utts + 1] */
    uint16_t *senid;    /* [n_nodes][4]: three senones, then the transition matrix id */
    int32_t *pen;       /* [n_nodes] log probability added on entry (logs2prob) */
    int32_t *parent;    /* [n_nodes] predecessor in the phone tree, -1 for word-initial nodes */
    uint32_t *info;     /* [n_nodes] bit 0 root, 1 leaf, 2 exit applies to every right context;
                           8..15 the CI phone shown to neighbours; 16..31 FSG state (roots: the
                           state they hang off, leaves that are not roots: unused) */
    uint64_t *ctxt;     /* [n_nodes] roots: left contexts served; leaves: right contexts served */
    int32_t *leaf_ord;  /* [n_nodes] ordinal among the utterance's leaves, -1 */
    int32_t *leaf_wid;  /* [n_leaves] dictionary word the leaf ends */
    int32_t *leaf_to;   /* [n_leaves] FSG state the word leads to */
    int32_t *leaf_node; /* [n_leaves] the leaf's node */
    int32_t *in_off;    /* [n_states + 1] leaves entering each state, into in_leaf */
    int32_t *in_leaf;   /* [n_in] leaf ordinals, by (left-context phone, ordinal) */
    /* alternates pronounced alike (twins): per member a record
     *   [L, n_ancestors, own element index, offset of its 3 x L rank / key buffers,
     *    L node indices: the ancestors root .. predecessor, then the members in chain order]
     * tw_off [n_utts + 1] into tw; twin_ref [n_nodes] = the node's record offset in its
     * utterance's part of tw, or -1; tw_rk [n_utts] = ints of rank buffers the utterance needs */
    int32_t n_tw;
    int32_t *tw, *tw_off, *twin_ref, *tw_rk;
    int32_t beam, pbeam, wbeam;
    uint64_t uid; /* unique per built set of graphs (never 0): the device copy's cache key */
    /* Grammar graphs only (ssw_grammar_graphs_build; NULL / 0 otherwise): one "utterance" per
     * grammar.  A state's entering list holds SLOTS: one per word-final HMM that leads into the
     * state, then one per (word-final HMM into a state s, closed null transition s -> state),
     * which is how fsg_search_null_prop's entries are folded in.  Slot indices are local to
     * their grammar (slot_off[state_off[g]] is its first). */
    int32_t n_slots, n_ls, n_sn;
    int32_t *g_start, *g_final; /* [n_utts] start and final state */
    int32_t *slot_off;   /* [n_states + 1] into the slot arrays */
    int32_t *slot_leaf;  /* [n_slots] leaf ordinal */
    int32_t *slot_pen;   /* [n_slots] the null transition's log probability >> 10; 0 for a word exit */
    int32_t *slot_null;  /* [n_slots] 1 for a null-hop slot */
    int32_t *slot_state; /* [n_slots] the state the slot enters */
    int32_t *ls_off;     /* [n_leaves + 1] a leaf's slots, into ls_slot: its word exit first */
    int32_t *ls_slot;    /* [n_ls] */
    int32_t *leaf_lscr;  /* [n_leaves] the link's log probability >> 10 (seg->lscr) */
    int32_t *leaf_filler;/* [n_leaves] fsg_model_is_filler of the link's word */
    int32_t *sn_off;     /* [n_utts + 1] null transitions out of the start state, into sn_* */
    int32_t *sn_to, *sn_pen; /* [n_sn] */
} ssw_fp_graphs_t;

/* a grammar as fsg_search_init leaves it (ssw_fsg_model.inc): the links of every state in the
 * order fsg_model_arcs walks them, words first, then the closed null transitions */
typedef struct ssw_fsg_link_s {
    int32_t from, to, logp, wid; /* logp: logs2prob (not shifted); wid: vocabulary index, -1 null */
} ssw_fsg_link_t;
typedef struct ssw_fsg_compiled_s {
    int32_t n_state, start, final, n_word, n_links;
    char **vocab;       /* [n_word] */
    int32_t *dict_wid;  /* [n_word] dictionary id, -1 when the dictionary lacks the word */
    uint8_t *is_sil;    /* [n_word] fsg_model_is_filler */
    ssw_fsg_link_t *links;
    int32_t *state_off; /* [n_state + 1] */
    float lw;
    double logbase;
} ssw_fsg_compiled_t;
ssw_fsg_compiled_t *ssw_fsg_compile(const ssw_fsg_t *f, const struct ssw_dict_s *d,
                                    const ssw_first_pass_config_t *cfg, int searched);
void ssw_fsg_compiled_free(ssw_fsg_compiled_t *c);
/* ssw_fsg_create as jsgf_build_fsg adds transitions (ssw_fsg_model.inc; used by ssw_jsgf.c) */
ssw_fsg_t *ssw_fsg_create_jsgf(const ssw_model_t *m, const struct ssw_dict_s *d, const char *name,
                               int32_t n_states, int32_t start, int32_t final, int32_t n_trans,
                               const int32_t *from, const int32_t *to, const float *prob,
                               const char *const *word);
ssw_fp_graphs_t *ssw_grammar_graphs_build(const ssw_model_t *m, const struct ssw_dict_s *d,
                                          const ssw_first_pass_config_t *cfg, int32_t n_fsgs,
                                          const ssw_fsg_t *const *fsgs);
ssw_fp_graphs_t *ssw_fp_graphs_build(const ssw_model_t *m, const struct ssw_dict_s *d,
                                     const ssw_first_pass_config_t *cfg, int32_t n_utts,
                                     const int32_t *word_off, const char *const *words);
void ssw_fp_graphs_free(ssw_fp_graphs_t *g);
/* Voice activity detection (ssw_vad.c: the object, the host path, the endpointer's replay;
 * ssw_host_vad.inc: the device calls).  The device workspace is the HIP side's: ssw_vad.c frees
 * it through dev_free, which the first device call sets. */
struct ssw_vad_s {
    int32_t mode, sample_rate, closest_rate, frame_size;
    int32_t nb_len;                                    /* the frame at 8 kHz: 80, 160 or 240 */
    int16_t overhead1, overhead2, individual, total;   /* the mode's thresholds at nb_len */
    void *d_state, *d_feat, *d_off;                    /* grow-only device buffers */
    size_t d_state_cap, d_feat_cap, d_off_cap;
    int64_t feat_frames;                               /* rows of d_feat the last call wrote; -1 none */
    int32_t spw;                                       /* streams per workgroup; 0 = by the batch's size */
    int32_t n_cus;                                     /* the device's compute units, asked once; 0 = not yet */
    void (*dev_free)(struct ssw_vad_s *);
};
struct ssw_endpoints_s {
    int32_t n_streams;
    int32_t *seg_off; /* [n_streams + 1] */
    ssw_endpoint_seg_t *segs;
};
/* the replay of ssw_endpoints_from_decisions per stream: decisions of stream u at
 * is_speech[frame_off[u] .. frame_off[u + 1]), its tail (samp_off[u + 1] - samp_off[u]) %
 * frame_size samples.  NULL and ssw_set_error. */
ssw_endpoints_t *ssw_endpoints_replay(const ssw_vad_t *v, double window, double ratio,
                                      const int8_t *is_speech, const int32_t *frame_off,
                                      const int64_t *tail, int32_t n_streams);
/* frame_off_out [n_streams + 1] of a batch, or -1 and ssw_set_error (bad offsets, too many frames) */
int ssw_vad_frame_offsets(const ssw_vad_t *v, const int64_t *samp_off, int32_t n_streams,
                          int32_t *frame_off_out);

int ssw_host_threads(void);
/* fn(arg, k) for k in [0, n_chunks) on a persistent pool of host threads + the caller */
void ssw_parallel_for(int n_chunks, void (*fn)(void *arg, int chunk), void *arg);

#ifdef __cplusplus
}
#endif
#endif
