"""MI355X-native SoundSwallower acoustic hot path: GMM senone scoring + forced alignment.

The compute lives in `libssw_amd.so` (C host code + hand-written gfx950 HIP kernels) behind the
C ABI of `include/ssw_amd.h`; this package is the thin host mirror used by tests and bench.
"""
from .api import (CMN_TYPES, Fe, Feat, FeatConfig, SswCmnState, CompactPlan, FirstPassPlan, Fsg, GrammarPlan, Jsgf, RecognitionSet, grammar_search_batch,
                  recognize_align_audio_batch, recognize_align_batch, recognize_align_batch_active,
                  recognize_audio_batch, recognize_batch, recognize_batch_active, INT_MAX, SCORER_MS, SCORER_PTM, SCORER_S2_SEMI, SSW_DEVICE_NONE, Lexicon, Mllr, Model, MsMgau, PtmMgau, S2SemiMgau,
                  StateAlignSearch, SswError, Texts, align_audio_batch, align_text_batch, align_text_batch_active, forced_align_batch, forced_align_planned, forced_alignment, fe_frame_counts, fe_frame_counts_at, model_dir,
                  Endpoints, Vad, endpoint_audio_batch, ENDPOINT_SEG_DTYPE, VAD_STATE_DTYPE)
from .synth import lcg_uniform, synth_features, synth_alignment_task

__all__ = ["Model", "Mllr", "Fe", "Feat", "FeatConfig", "SswCmnState", "CMN_TYPES", "CompactPlan", "PtmMgau", "MsMgau", "S2SemiMgau", "Lexicon", "StateAlignSearch", "SswError", "FirstPassPlan", "Fsg", "GrammarPlan", "Jsgf", "RecognitionSet", "grammar_search_batch", "recognize_batch", "recognize_batch_active", "recognize_audio_batch", "recognize_align_batch", "recognize_align_batch_active", "recognize_align_audio_batch", "Texts", "align_audio_batch", "align_text_batch", "align_text_batch_active", "forced_align_batch", "forced_align_planned", "forced_alignment", "fe_frame_counts", "fe_frame_counts_at", "model_dir", "SCORER_PTM",
           "SCORER_MS", "SCORER_S2_SEMI", "SSW_DEVICE_NONE", "INT_MAX", "lcg_uniform", "synth_features", "synth_alignment_task", "Vad", "Endpoints", "endpoint_audio_batch",
           "VAD_STATE_DTYPE", "ENDPOINT_SEG_DTYPE"]
