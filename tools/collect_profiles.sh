#!/bin/bash
# Everything the round's profiles/ files come from, in one call ON the GPU box:
#   gpurun --timeout 3000 -- 'bash tools/collect_profiles.sh r06'
# Writes gpurun_out/<tag>/; copy what is to be judged into profiles/<tag>_* afterwards
# (tools/collect_profiles.sh does not touch profiles/).  rocprofv3 gets `python3 <script>` directly
# after `--` (no shell, no env in between) and --pmc passes are never combined with other traces.
tag=${1:-r06}
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/$tag
mkdir -p $O
export TMPDIR=/tmp
cd $R
if [ "$2" != "notests" ]; then
  timeout 600 python -m pytest tests -x -q -m gpu > $O/pytest.log 2>&1
  grep -E "passed|failed" $O/pytest.log | tail -2
fi
timeout 600 python bench.py --full > $O/bench_line.json 2> $O/bench.err
cd /tmp
prof() {  # name, then the program
  local name=$1; shift
  timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$name -o $name -- "$@" > $O/${name}_under_rocprof.json 2> $O/${name}_rocprof.err
  find $O/prof_$name -name "*kernel_stats.csv" -exec cp {} $O/${name}_kernel_stats.csv \;
  find $O/prof_$name -name "*kernel_trace.csv" -delete
}
prof headline python3 $R/bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-align --no-extra
prof full python3 $R/bench.py --steps 200 --warmup 20 --full --no-cpu-baseline
prof config4 python3 $R/tools/bench_ms.py
prof config3_align python3 $R/tools/bench_align.py
prof config5_align python3 $R/tools/bench_align.py --utts 2048 --reps 2
prof align_active python3 $R/tools/bench_align_active.py --reps 2
prof first_pass python3 $R/tools/bench_first_pass.py --reps 5
prof page python3 $R/tools/bench_page.py
# round 6: the default configuration from text as a batch (speculation and proof)
prof fpa python3 $R/tools/bench_first_pass_active.py --reps 3
cd $R
timeout 900 python3 tools/pmc_pass.py $tag > $O/pmc.log 2>&1
tail -2 $O/pmc.log
timeout 300 python tools/bench_page.py > $O/page.json 2>/dev/null
timeout 300 python tools/bench_frame_sync.py > $O/frame_sync.json 2>/dev/null
timeout 300 python tools/bench_first_pass.py --reps 5 > $O/first_pass.json 2>/dev/null
timeout 300 python tools/bench_ms.py > $O/config4_ms.json 2>/dev/null
timeout 300 python tools/bench_align.py > $O/config3_align.json 2>/dev/null
timeout 300 python tools/bench_align.py --utts 2048 > $O/config5_align.json 2>/dev/null
SSW_JOB_ROWS=full SSW_ALIGN_BT=0 timeout 300 python tools/bench_align.py --utts 2048 > $O/config5_align_full_rows_full_tokens.json 2>/dev/null
timeout 300 python tools/bench_align_active.py > $O/align_active.json 2>/dev/null
timeout 300 python tools/bench_align_active.py --ms > $O/align_active_ms.json 2>/dev/null
timeout 300 python tools/bench_host_boundary.py > $O/host_boundary.json 2>/dev/null
SSW_ALIGN_TIMING=1 timeout 300 python tools/bench_first_pass_active.py --reps 3 > $O/fpa_synth.json 2> $O/fpa_synth_rounds.txt
timeout 300 python tools/bench_first_pass_active.py --real --utts 240 > $O/fpa_real.json 2>/dev/null
# texts of ~300 words (2,940 phone-tree HMMs): the sliding-window kernel, which texts beyond 1,024
# HMMs take since round 5 (the register instances with 2 and 4 HMMs per thread, the ones with
# scratch, lost to it from ~1,200 HMMs up and were removed: VERDICT r4 weak 7); the second line
# forces the window kernel and must read the same
timeout 300 python tools/bench_first_pass.py --utts 32 --words 300 --frames 12000 --reps 2 > $O/first_pass_300_words.json 2>/dev/null
SSW_FP_KERNEL=big timeout 300 python tools/bench_first_pass.py --utts 32 --words 300 --frames 12000 --reps 2 > $O/first_pass_300_words_window_kernel.json 2>/dev/null
# counters of the alignment kernel on compact rows + byte tokens, and on the round-4 form
timeout 900 python3 tools/pmc_cmd.py gpurun_out/$tag/align_pmc_2048.json 'viterbi_align\w+|ptm_senone_kernel|ptm_topn_mfma_kernel' -- python3 tools/bench_align.py --utts 2048 --reps 1 > $O/align_pmc_2048.log 2>&1
timeout 900 python3 tools/pmc_cmd.py gpurun_out/$tag/align_pmc_256.json 'viterbi_align\w+' -- python3 tools/bench_align.py --utts 256 --reps 1 > $O/align_pmc_256.log 2>&1
timeout 900 python3 tools/pmc_cmd.py gpurun_out/$tag/align_active_pmc.json 'senone_active2_kernel|viterbi_align\w+' -- python3 tools/bench_align_active.py --reps 1 > $O/align_active_pmc.log 2>&1
timeout 900 python3 tools/pmc_cmd.py gpurun_out/$tag/fpa_pmc.json 'senone_listed_kernel|fpa_plan_kernel|fpa_compare_kernel|first_pass_kernel|ptm_topn_mfma_kernel' -- python3 tools/bench_first_pass_active.py --reps 1 > $O/fpa_pmc.log 2>&1
# the senone kernel's selectable shapes on the headline workload
timeout 600 bash tools/bench_sen_shapes.sh $tag > $O/sen_shapes.log 2>&1
rm -rf $R/gpurun_out/pmc_align_pmc_2048 $R/gpurun_out/pmc_align_pmc_256 $R/gpurun_out/pmc_align_active_pmc $R/gpurun_out/pmc_fpa_pmc
ls $O
