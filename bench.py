#!/usr/bin/env python3
"""bench.py -- senone-frames/s of the PTM scoring hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A step is one pass of the hot path (ssw_score_batch: density/top-N kernel + senone kernel)
over one batch of synthetic features already resident in HBM: BASELINE.json configs[1],
4096 frames of 39-dim features as 16 utterances x 256 frames, en-us PTM model.  With N > 1
(one rank per GPU: launched by torch.distributed.run, or -- when WORLD_SIZE is not in the
environment -- by this script itself, which starts the N ranks as child processes before it has
touched the GPU) every rank scores its own shard of utterances -- the path partitions by
utterance, there is no data-path collective -- and the reported value is the whole-job rate over
the max-over-ranks time (weak scaling).

A plain run sets up, warms up, times the K steps and prints ONE JSON line on rank 0: `value`,
`ms_per_step` (wall milliseconds of one timed step) and `roofline`, which is derived from the
timed region itself (two HIP events on the launch stream around it).  --dump-outputs DIR also
writes what the last timed step computed (rank 0's senone scores) to DIR as float32 .npy files;
the inputs are seeded, so two builds can be compared output for output.

--full adds what takes runs of its own, each in the same line:
  `kernels`      the per-kernel split, from a separate pass with HIP events between the launches;
  `cpu_baseline` the CPU oracle timed on a bounded sample of the same workload on the host
                 cores of this box, one core and all cores (N = 1 only);
  `config5`      BASELINE.json configs[4] at every N: 2048 utterances x 1000 frames x 150 phones
                 dealt over the N ranks, each rank scoring and force-aligning its shard, ONE
                 gather of the final alignments over RCCL; job utterance-frames/s, align RTF,
                 gather_ms and a CRC of the gathered alignments that does not depend on N;
  `batch_16384`, `batch_65536`, `real_features`, `align`, `text_align`, `text_align_default_config`  (N = 1 only) the same scoring step
                 at 65,536 frames, on features of a real recording, and BASELINE configs[2]
                 from phone strings and from text;
  `config4`      (N = 1 only) BASELINE configs[3]: the ms scorer on fr-fr, 8192 frames per step.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_UTTS = 16
UTT_FRAMES = 256
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak, MI355X_MICROARCH.md
VALU_PEAK_TOPS = 78.6          # vector fp32 peak with an FMA counted once
# reference work per frame: (densities + re-scored top-N codewords) x dimensions x (sub, mul,
# mul, sub): 864,864 for en-us PTM
N_SIMD = 1024                   # 256 CUs x 4 SIMDs
CLOCK_HZ = 2.4e9
DUMP_BYTES = 60_000_000        # --dump-outputs writes at most this much (under 64 MB)
PMC_FILE = "r06_pmc.json"      # rocprofv3 --pmc passes of this step (tools/pmc_pass.py); only
                               # quoted when its kernel_src_sha equals this tree's


def kernel_src_sha() -> str:
    """Hash of everything libssw_amd.so is compiled from: ties a profile to the code it measured."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "soundswallower_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".c", ".h", ".hip", ".inc")) or name == "Makefile":
            with open(os.path.join(csrc, name), "rb") as fh:
                h.update(name.encode() + b"\0" + fh.read())
    with open(os.path.join(ROOT, "include", "ssw_amd.h"), "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()[:16]


def algorithmic_bytes(n_sen, n_feat, topn, n_cb, n_density, veclen_total, batch):
    """SURVEY.md 8(d) touched-bytes accounting, per frame, and its split over the two kernels."""
    feat_b = 4 * veclen_total
    out_b = 2 * n_sen
    mixw_b = n_sen * n_feat * topn
    gauss_block = n_cb * n_density * (2 * veclen_total + n_feat) * 4
    topn_b = n_cb * n_feat * (topn + 4 * topn)          # packed cw + int32 scores between kernels
    whole = feat_b + out_b + mixw_b + gauss_block / batch
    return {"path": whole,
            "topn_kernel": feat_b + gauss_block / batch + topn_b,
            "senone_kernel": topn_b + mixw_b + out_b}


def align_config3(ssw, model, means, torch, n_utts=256, n_frames=1000, n_phones=150, reps=3):
    """BASELINE configs[2]: score and force-align 256 synthetic utterances x 1000 frames x 150
    phones (the "align RTF" part of the metric); best of `reps` passes."""
    from soundswallower_amd.synth import synth_alignment_task
    sseq = model.table("sseq").reshape(-1, 3)
    pssid, ptmat = model.table("phone_ssid"), model.table("phone_tmat")
    feats = np.concatenate([ssw.synth_features(means, n_frames, 12345 + u) for u in range(n_utts)])
    senid, tmat = [], []
    for u in range(n_utts):
        s_, t_, _ = synth_alignment_task(sseq, pssid, ptmat, model.n_ciphone, n_phones, 777 + u)
        senid.append(s_)
        tmat.append(t_)
    senid, tmat = np.concatenate(senid), np.concatenate(tmat)
    frame_off = (np.arange(n_utts + 1) * n_frames).astype(np.int32)
    phone_off = (np.arange(n_utts + 1) * n_phones).astype(np.int32)
    total = n_utts * n_frames
    d_feats = torch.from_numpy(feats).cuda()
    d_scr = torch.empty((total, model.n_sen), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    best = None
    t_spin = time.perf_counter()     # the GPU idled while the host made the inputs (see spin_up)
    while time.perf_counter() - t_spin < 0.3:
        model.score_batch_device(d_feats, total, frame_off, d_scr, stream)
        torch.cuda.synchronize()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.score_batch_device(d_feats, total, frame_off, d_scr, stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st, status = model.align_batch(d_scr.data_ptr(), frame_off, phone_off, senid, tmat)
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    tiles = all(st[phone_off[u] * 3:phone_off[u + 1] * 3, 1].sum() == n_frames
                for u in range(n_utts) if status[u] == 0)
    # the same job through compact score rows (round 5: the plan of the alignments is built
    # inside the timed region; the scorer stores each utterance's own states only)
    d_c = torch.empty((n_utts * n_frames * ((3 * n_phones + 1) & ~1),), dtype=torch.int16, device="cuda")
    cbest, st_c = None, None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = model.compact_plan(frame_off, phone_off, senid, stream=stream)
        model.score_batch_compact(d_feats, plan, d_c, stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st_c, status_c = model.align_batch_compact(plan, d_c, tmat)
        t2 = time.perf_counter()
        plan.free()
        if cbest is None or t2 - t0 < cbest[0]:
            cbest = (t2 - t0, t1 - t0, t2 - t1)
    return {"workload": f"{n_utts} utterances x {n_frames} frames x {n_phones} phones, en-us: PTM "
                        f"scoring + forced alignment (BASELINE configs[2])",
            "score_ms": best[1] * 1e3, "align_ms": best[2] * 1e3,
            "rtf": best[0] / (total / 100.0), "utt_frames_per_s": total / best[0],
            "aligned": int((status == 0).sum()), "alignments_tile_their_utterances": bool(tiles),
            "compact_rows": {"score_ms": cbest[1] * 1e3, "align_ms": cbest[2] * 1e3,
                             "rtf": cbest[0] / (total / 100.0), "utt_frames_per_s": total / cbest[0],
                             "same_alignments_as_full_rows": bool(np.array_equal(st_c, st)
                                                                  and np.array_equal(status_c, status))}}


# ---- CPU baseline (the only part of this file that touches oracle/) -----------------------
def cpu_worker(model_dir, seeds, seconds):
    """One host core (`python bench.py --cpu-worker ...`): its own oracle model, its own
    utterances, for ~`seconds`; prints frames and seconds."""
    from oracle import oracle as O
    from soundswallower_amd.synth import read_raw_means, synth_features
    m = O.Model(model_dir)
    means = read_raw_means(model_dir)
    utts = [synth_features(means, UTT_FRAMES, s) for s in seeds]
    m.ptm_score_utt(utts[0][:8])                  # page everything in before the clock starts
    n_done, k, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        m.ptm_score_utt(utts[k % len(utts)])      # history reset per utterance, as the batch API
        n_done += UTT_FRAMES
        k += 1
    print(json.dumps({"frames": n_done, "seconds": time.perf_counter() - t0}), flush=True)


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(model_dir, one_core_s=6.0, all_core_s=8.0):
    """SURVEY 8(d) / BASELINE.md section 3: the reference is single-threaded, so the all-core
    figure is N independent processes, each with its own model, each scoring its own utterances
    of the bench workload (16 utterances x 256 frames, seeds 12345 + u, dealt over the processes
    and cycled).  Timed on the host cores of this box with the CPU oracle (bit-identical
    restatement of the reference path; /root/reference does not exist on the GPU box).
    Runs BEFORE this process touches the GPU; the workers are child processes."""
    import subprocess
    try:
        n_cores = len(os.sched_getaffinity(0))
    except AttributeError:
        n_cores = os.cpu_count() or 1

    def run(n_proc, seconds):
        def seeds(p):  # a disjoint slice of the 16 utterances per process (shared beyond 16)
            return ([12345 + u for u in range(N_UTTS) if u % n_proc == p]
                    or [12345 + p % N_UTTS])
        procs = [subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--cpu-worker", model_dir, str(seconds)]
            + [str(x) for x in seeds(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
            text=True) for p in range(n_proc)]
        frames, rate, longest = 0, 0.0, 0.0
        for p in procs:
            so, se = p.communicate(timeout=seconds + 240)
            if p.returncode != 0:
                raise RuntimeError("cpu_baseline worker failed: " + se[-400:])
            r = json.loads(so.strip().splitlines()[-1])
            frames += r["frames"]
            rate += r["frames"] / r["seconds"]
            longest = max(longest, r["seconds"])
        return frames, rate, longest

    f1, r1, t1 = run(1, one_core_s)
    fa, ra, ta = run(n_cores, all_core_s) if n_cores > 1 else (f1, r1, t1)
    return {"value": ra, "unit": "frames/s", "cores": n_cores, "kind": "port",
            "per_core": r1, "all_core": ra, "cpu_model": cpu_model_name(),
            "sample": f"one process for {t1:.1f} s ({f1} frames), then {n_cores} independent "
                      f"processes side by side for {ta:.1f} s ({fa} frames in all; the rate is "
                      f"the sum of the processes' own rates), each with its own model, cycling "
                      f"over its share of the bench batch's 16 utterances x {UTT_FRAMES} "
                      f"frames (CPU oracle oracle/ssw_oracle.c, a scalar C port of the reference "
                      f"path, bit-identical to it on the golden fixtures; gcc -O2 "
                      f"-ffp-contract=off)"}


# ---- the scoring step -----------------------------------------------------------------------
class ScoreStep:
    def __init__(self, torch, model, feats, utt_off):
        self.model, self.utt_off = model, utt_off
        self.n_frames = feats.shape[0]
        self.d_feats = torch.from_numpy(feats).cuda()
        self.d_out = torch.empty((self.n_frames, model.n_sen), dtype=torch.int16, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        self.model.score_batch_device(self.d_feats, self.n_frames, self.utt_off, self.d_out,
                                      self.stream)

    def kernel_ms(self, n):
        """Per-kernel durations of one step from HIP events recorded on the launch stream."""
        self.model.set_kernel_timing(True)
        k_ms = np.zeros(2)
        for _ in range(n):
            self()
            k_ms += np.array(self.model.kernel_timing())
        self.model.set_kernel_timing(False)
        return k_ms / n


def spin_up(torch, step, seconds=0.5):
    """~0.5 s of the step itself before the warm-up steps: a fresh box's GPU takes longer than
    a few 0.1 ms steps to reach its working clock."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50):
            step()
        torch.cuda.synchronize()


def dump_outputs(out_dir, scores):
    """--dump-outputs: the senone scores [frames][senones] the last timed step left in HBM (what a
    caller of ssw_score_batch receives) as DIR/senone_scores.npy, float32 (int16 converts
    exactly), and the frame index of each row as DIR/senone_scores_frames.npy.  A whole step of
    en-us is 80 MB as float32: beyond DUMP_BYTES the rows are a fixed, seeded sample of frames."""
    n, n_sen = scores.shape
    rows = np.arange(n)
    cap = DUMP_BYTES // (4 * n_sen + 8)
    if n > cap:
        rows = np.sort(np.random.default_rng(0).choice(n, size=cap, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "senone_scores.npy"), scores[rows].astype(np.float32))
    np.save(os.path.join(out_dir, "senone_scores_frames.npy"), rows.astype(np.float64))


def timed_steps(torch, dist, backend, step, warmup, steps):
    """(host seconds over the K steps, max over ranks; this rank's device milliseconds over the
    same K steps from two HIP events on the launch stream, recorded before the first launch and
    after the last -- the step's kernels back to back with nothing of the host in between)"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)   # (the steps are launched on torch's current
    ev1 = torch.cuda.Event(enable_timing=True)   # stream: ScoreStep.stream)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        step()
    ev1.record()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    region_ms = ev0.elapsed_time(ev1)
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, region_ms


def self_launch(n_ranks):
    """`python bench.py --gpus N` without a launcher: this process has not touched the GPU (no
    torch import, no HIP call), so it may start the N ranks itself -- fresh child processes with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, the same command line -- relay
    rank 0's JSON line and exit non-zero if any rank does."""
    import socket
    import subprocess
    # (the port is free now and claimed by rank 0's store a moment later; a caller that needs a
    # fixed one sets SSW_BENCH_MASTER_PORT)
    port = int(os.environ.get("SSW_BENCH_MASTER_PORT", "0"))
    if port == 0:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_ranks),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                   LOCAL_WORLD_SIZE=str(n_ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL,
                                      text=True))
    # Rank 0's stdout is drained on a thread while ALL ranks are polled: a rank that dies early
    # (bad device, import error, out of memory) would otherwise leave rank 0 waiting in
    # init_process_group or a collective until the process group's own timeout, minutes later
    # (ADVICE r5).  The first non-zero exit ends the job: the rest are terminated.
    import threading
    rc, chunks = 0, []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    limit = float(os.environ.get("SSW_BENCH_LAUNCH_TIMEOUT", "3600"))
    t_end = time.time() + limit
    try:
        pending = list(procs)
        while pending and not rc:
            for p_ in list(pending):
                code = p_.poll()
                if code is not None:
                    pending.remove(p_)
                    if code and not rc:
                        rc = code
                        sys.stderr.write(f"bench.py: rank {procs.index(p_)} exited with code "
                                         f"{code}; stopping the other ranks\n")
            if time.time() > t_end:
                sys.stderr.write(f"bench.py: ranks still running after {limit:.0f} s\n")
                rc = rc or 1
            if pending and not rc:
                time.sleep(0.05)
    finally:
        for p_ in procs:                             # exactly the processes started above
            if p_.poll() is None:
                p_.terminate()
        for p_ in procs:
            try:
                p_.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p_.kill()
                p_.wait()
        reader.join(timeout=10)
    out0 = "".join(c or "" for c in chunks)
    # ONE JSON line on stdout: whatever else rank 0's libraries printed there (gloo's "Rank 0 is
    # connected to ..." for one) goes to stderr
    line = ""
    for ln in out0.splitlines():
        if ln.startswith("{") and ln.rstrip().endswith("}"):
            line = ln
        elif ln.strip():
            sys.stderr.write(ln + "\n")
    if line:
        sys.stdout.write(line + "\n")
    sys.stdout.flush()
    if rc:
        raise SystemExit(f"bench.py: a rank of the self-launched {n_ranks}-rank job exited with "
                         f"code {rc}")
    if not line:
        raise SystemExit("bench.py: rank 0 printed no line")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":   # child of cpu_baseline()
        return cpu_worker(sys.argv[2], [int(x) for x in sys.argv[4:]], float(sys.argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="en-us")
    ap.add_argument("--full", action="store_true",
                    help="also the per-kernel split, the CPU baseline, config5 and (N = 1) the "
                         "larger batches, real features and configs 3 and 4; the --no-* options "
                         "below leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's senone scores (rank 0) to DIR as .npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-align", action="store_true",
                    help="skip the config-3 / text / config-5 alignment jobs")
    ap.add_argument("--no-extra", action="store_true",
                    help="skip the 65,536-frame and real-feature scoring lines")
    ap.add_argument("--utts", type=int, default=N_UTTS,
                    help="utterances (x256 frames) per GPU per step; the default is BASELINE.json "
                         "configs[1], 4096 frames")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import soundswallower_amd as ssw
    mdir = ssw.model_dir(args.model)
    cpu = None
    if args.full and not args.no_cpu_baseline and world == 1:   # N = 1 only; before any GPU call
        cpu = cpu_baseline(mdir)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the scoring path has no CPU fallback")
    # SSW_BENCH_BACKEND=gloo + SSW_BENCH_DEVICE=0 let several ranks share one GPU, to exercise the
    # multi-rank control flow on a 1-GPU box; the driver's runs use nccl (= RCCL), one GPU per rank
    backend = os.environ.get("SSW_BENCH_BACKEND", "nccl")
    if "SSW_BENCH_DEVICE" in os.environ:
        local_rank = int(os.environ["SSW_BENCH_DEVICE"])
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    from soundswallower_amd import _lib, jobs
    from soundswallower_amd.parallel import shard_utterances
    from soundswallower_amd.synth import read_raw_means as raw_means

    if rank == 0:          # one rank compiles (a no-op when the .so is current); the rest wait
        _lib.build()
    if dist:
        dist.barrier()
    model = ssw.Model(mdir, config={"device": local_rank})
    means = raw_means(mdir)

    # this rank's shard of the global utterance list (weak scaling: N_UTTS per rank)
    global_utts = list(range(args.utts * world))
    mine = shard_utterances([UTT_FRAMES] * len(global_utts), world)[rank]
    feats = np.concatenate([ssw.synth_features(means, UTT_FRAMES, 12345 + u) for u in mine])
    utt_off = (np.arange(len(mine) + 1) * UTT_FRAMES).astype(np.int32)
    n_frames = feats.shape[0]

    step = ScoreStep(torch, model, feats, utt_off)
    if not os.environ.get("SSW_BENCH_NO_SPIN"):   # (tools/pmc_pass.py: keep the trace short)
        spin_up(torch, step, float(os.environ.get("SSW_BENCH_SPIN", "0.5")))
    elapsed, region_ms = timed_steps(torch, dist, backend, step, args.warmup, args.steps)
    flagged, pairs = model.last_stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step.d_out.cpu().numpy())
    k_ms = step.kernel_ms(max(1, min(args.steps, 50))) if args.full else None

    # BASELINE configs[4] on every rank count (the multi-GPU part of the metric): collective
    c5 = None
    if args.full and not args.no_align and args.model == "en-us":
        # the gather goes through the library's C entry point (ssw_gather_alignments over its own
        # RCCL communicator) when the ranks are on GPUs of their own; SSW_GATHER=torch, a failed
        # communicator set-up, or the gloo shared-GPU test mode use torch.distributed instead
        comm, how = None, "none (one rank)"
        if world > 1:
            how = "rccl (torch.distributed nccl)" if backend == "nccl" else backend
            if backend == "nccl" and os.environ.get("SSW_GATHER", "c") == "c":
                from soundswallower_amd.parallel import RcclComm
                try:
                    comm = RcclComm(dist, world, rank, local_rank)
                    how = "rccl (ssw_gather_alignments, C ABI)"
                except Exception as e:      # noqa: BLE001 -- reported in the line
                    how += f" [C communicator unavailable: {e}]"
            ok = torch.tensor([1 if comm is not None else 0],
                              device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)   # all ranks take the same route
            if int(ok.item()) == 0 and comm is not None:
                comm.close()
                comm = None
                how = "rccl (torch.distributed nccl) [C communicator missing on another rank]"
        c5 = jobs.run_config5(model, means, dist, rank, world,
                              torch.device("cuda", local_rank) if backend == "nccl" else None,
                              comm=comm, reps=3)   # best of three: the job's host side (250
        # launches, the alignment's set-up) is exposed to whatever else the box's host is doing
        c5["gather_backend"] = how
        # the ranks RCCL itself counts in the library's communicator (ncclCommCount)
        c5["rccl_ranks"] = comm.count() if comm is not None else None
        if comm is not None:
            comm.close()

    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return

    ab = algorithmic_bytes(model.n_sen, model.n_feat, model.topn, model.n_cb, model.n_density,
                           model.veclen_total, n_frames)
    REF_OPS_PER_FRAME = model.n_cb * (model.n_density + model.topn) * model.veclen_total * 4
    names = ("topn_kernel", "senone_kernel")
    total_frames = n_frames * world * args.steps
    fps = total_frames / elapsed
    # roofline of the hot path = the launches of one step (top-N pass, senone pass);
    # algorithmic bytes = SURVEY 8(d)'s 72,345 B/frame x frames per launch set.  Duration: the
    # device time of the timed region's K steps (two HIP events on the launch stream around
    # them) / K, i.e. the two kernels' launch durations plus the ~1 us between dependent
    # launches.  (Rounds 1-3 summed per-kernel event pairs of a separate instrumented pass: an
    # event between two launches costs ~2 us of its own, 5-10 % of a 35 us kernel -- those stay in
    # `kernels` as the split, marked; profiles/r04_kernel_stats.csv has rocprofv3's durations.)
    path_ms = region_ms / args.steps
    ms_per_step = elapsed / args.steps * 1e3
    # frac = frames/s (per GPU) x algorithmic bytes per frame / peak, i.e. on the WALL
    # time of the K steps (what the driver recomputes); frac_kernels = the same bytes over the
    # device time of the same K steps (two HIP events on the launch stream around them)
    achieved = ab["path"] * n_frames / (ms_per_step * 1e-3) / 1e9
    achieved_k = ab["path"] * n_frames / (path_ms * 1e-3) / 1e9
    sha = kernel_src_sha()
    traffic = valu_instr = None
    traffic_source = "not measured for this build (no profiles/%s)" % PMC_FILE
    tfile = os.path.join(ROOT, "profiles", PMC_FILE)
    if os.path.exists(tfile) and n_frames == 4096 and args.model == "en-us":
        with open(tfile) as fh:      # PMC counters cannot be read from inside this process:
            pmc = json.load(fh)      # committed rocprofv3 passes over this same command
        if pmc.get("kernel_src_sha") == sha:
            traffic = pmc["hbm_bytes"]
            valu_instr = pmc["valu_wave_instr_per_step"]
            traffic_source = (f"profiles/{PMC_FILE}: rocprofv3 --pmc passes of this command on "
                              f"this build (kernel_src_sha {sha}); FETCH_SIZE doubled per "
                              f"MI355X_MICROARCH.md (HBM section) for the wide streaming reads")
        else:
            traffic_source = (f"profiles/{PMC_FILE} was taken on kernel_src_sha "
                              f"{pmc.get('kernel_src_sha')}, this build is {sha}: not quoted")
    out = {
        "metric": "senone-frames/sec (en-us PTM)",
        "value": fps,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "scaling_note": "value = weak scaling of the scoring step (4096 frames per rank, no "
                        "data-path collective); config5 = the STRONG-scaling job of BASELINE "
                        "configs[4] (2048 utterances dealt over the ranks, one gather)",
        "vs_baseline": None,
        "dtype": "f32+i32",
        "data": "synthetic",
        "config": {"workload": f"PTM senone scoring, {args.model}, {args.utts} utterances x "
                               f"{UTT_FRAMES} frames = {n_frames} frames per GPU per step, "
                               f"39-dim features resident in HBM, compallsen=yes, topn=4",
                   "senones": model.n_sen, "codebooks": model.n_cb,
                   "parallelism": f"utt-shard x{world}"},
        # the graded figure: SURVEY 8(d)'s touched bytes per frame against the HBM peak (what
        # north_star's "50 % of HBM roofline" is measured in): frac x peak x ms_per_step =
        # algorithmic_bytes_per_frame x frames.  `bound` names the roof the figure is quoted
        # against; what actually limits the kernels is vector-instruction issue (binding_roof,
        # valu_roofline) and their real HBM traffic is `traffic` (hbm_traffic_frac of the peak)
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "frac_kernels": achieved_k / HBM_PEAK_GBS, "achieved_kernels": achieved_k,
                     "traffic": traffic,
                     "hbm_traffic_frac": (traffic / (path_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                                          if traffic else None),
                     "traffic_source": traffic_source,
                     "graded_metric": "touched (algorithmic) bytes per frame x frames/s against "
                                      "the HBM peak, on the wall time of the timed steps",
                     "binding_roof": "valu_issue (see valu_roofline and valu_frac)",
                     "kernel": "PTM path of one step: ptm_topn_mfma (or ptm_topn_frames, SSW_SCAN=fma) "
                               "+ ptm_senone",
                     "kernel_ms": path_ms, "algorithmic_bytes_per_frame": ab["path"],
                     "kernel_src_sha": sha,
                     "note": "achieved = ALGORITHMIC (touched-bytes, SURVEY 8(d)) GB/s, not HBM "
                             "traffic: 61.5 of the 72 KB/frame are gathers from the 2 MB mixture-"
                             "weight table, which L2 serves; the path is VALU-issue bound "
                             "(DESIGN.md section 5)"},
        # SURVEY 8(d)'s second number: the reference's arithmetic per frame (864,864 non-fused
        # fp32 operations for en-us PTM; the matrix-core scan does most of it elsewhere, so this
        # is a rate of REFERENCE work, not of instructions issued) against the vector unit's
        # non-fused peak
        "valu_roofline": {"bound": "valu", "achieved": fps / world * REF_OPS_PER_FRAME / 1e12,
                          "peak": VALU_PEAK_TOPS, "unit": "Top/s (non-fused fp32, reference work)",
                          "frac": fps / world * REF_OPS_PER_FRAME / 1e12 / VALU_PEAK_TOPS},
        # share of the SIMDs' vector issue slots the step uses at 4 cycles per wave64 instruction
        # (SQ_INSTS_VALU from the PMC file), at the nominal 2.4 GHz (the chip holds less under
        # this load, so the true share is higher)
        "valu_frac": (valu_instr * 4.0 / N_SIMD / CLOCK_HZ / (path_ms * 1e-3)
                      if valu_instr else None),
        "exact_pass_share": flagged / max(pairs, 1),
        # the matrix-core scan's load-time self-test on this device (ssw_model_info_t)
        "scan": {"mode": "matrix cores" if model.scan_mode == 1 else "vector unit",
                 "mfma_selftest": model.mfma_selftest,
                 "mfma_selftest_worst_u": model.mfma_selftest_worst_u,
                 "mfma_selftest_ms": model.mfma_selftest_ms},
    }
    if k_ms is not None:
        per_kernel = {
            nm: {"ms": float(k_ms[i]), "algorithmic_bytes_per_frame": ab[nm],
                 "achieved_GBps": ab[nm] * n_frames / (k_ms[i] * 1e-3) / 1e9,
                 "hbm_frac": ab[nm] * n_frames / (k_ms[i] * 1e-3) / 1e9 / HBM_PEAK_GBS}
            for i, nm in enumerate(names)}
        per_kernel["senone_kernel"]["note"] = (
            "hbm_frac > 1 is an accounting artefact, not skipped work: 61.5 of this kernel's "
            "algorithmic KB/frame are gathers from the 2 MB mixture-weight table, which the L2s "
            "serve; its real HBM traffic is roofline.traffic")
        out["kernels"] = dict(per_kernel, note="per-kernel split from a separate pass with a HIP "
                              "event between the two launches (each event adds ~2 us to what it "
                              "brackets); their sum exceeds roofline.kernel_ms by that overhead")
    if c5 is not None:
        out["config5"] = c5
    if args.full and world == 1 and args.model == "en-us" and not args.no_extra:
        # north_star says "batch >= 4096 frames": the same step at 16,384 frames per launch (the
        # size at which a frame costs least: DESIGN.md section 5) and at 65,536 (scored in four
        # pieces of 16,384).  roofline_frac: from the wall time of the steps, like the headline's
        # `frac` as the driver recomputes it; roofline_frac_kernels: from the kernels' own time
        for big_utts in (64, 256):
            bf = np.concatenate([ssw.synth_features(means, UTT_FRAMES, 12345 + u) for u in range(big_utts)])
            boff = (np.arange(big_utts + 1) * UTT_FRAMES).astype(np.int32)
            big = ScoreStep(torch, model, bf, boff)
            spin_up(torch, big, 0.3)   # the GPU idled while the host made the features (as for `value`)
            nst = 40 if big_utts == 64 else 20
            e, e_dev = timed_steps(torch, None, backend, big, 3, nst)
            bk = np.array([e_dev / nst])
            bab = algorithmic_bytes(model.n_sen, model.n_feat, model.topn, model.n_cb,
                                    model.n_density, model.veclen_total, big.n_frames)
            out[f"batch_{big.n_frames}"] = {
                "workload": f"the same step at {big.n_frames} frames per launch ({big_utts} x 256)",
                "frames_per_s": big.n_frames * nst / e, "ms_per_step": e / nst * 1e3,
                "kernel_ms": float(bk.sum()),
                "roofline_frac": bab["path"] * big.n_frames * nst / e / 1e9 / HBM_PEAK_GBS,
                "roofline_frac_kernels": bab["path"] * big.n_frames / (float(bk.sum()) * 1e-3) / 1e9 / HBM_PEAK_GBS}
            del big
        rf = real_features(ssw, model, torch)
        if rf is not None:
            out["real_features"] = rf
    if args.full and not args.no_align and world == 1 and args.model == "en-us":
        out["align"] = align_config3(ssw, model, means, torch)
        # the same job from TEXT: first pass (which fillers / alternates, word frames) + the
        # rest of decoder_alignment, tools/bench_first_pass.py
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import bench_first_pass
        lex = ssw.Lexicon(model, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
        out["text_align"] = bench_first_pass.run(ssw, model, lex, torch)
        # the same second pass in the reference's DEFAULT configuration (compallsen = no): one
        # ssw_align_batch_active call, tools/bench_align_active.py
        import bench_align_active
        try:
            out["align_default_config"] = bench_align_active.run(model)
        except Exception as e:      # noqa: BLE001 -- the headline line must still come out
            out["align_default_config"] = {"error": str(e)}
        # and the whole of decoder_alignment from text in that configuration (round 6): the first
        # pass by speculation and proof (ssw_first_pass_batch_active), then the second pass over
        # the growing active set -- tools/bench_first_pass_active.py, text_align's workload
        import bench_first_pass_active
        try:
            out["text_align_default_config"] = bench_first_pass_active.run(ssw, model, lex, torch,
                                                                           reps=2)
        except Exception as e:      # noqa: BLE001
            out["text_align_default_config"] = {"error": str(e)}
    if args.full and world == 1 and not args.no_extra:
        # BASELINE configs[3]: the ms scorer (ms_gauden + ms_senone kernels), fr-fr, 8192 frames
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import bench_ms
        try:
            out["config4"] = bench_ms.run()
        except Exception as e:      # noqa: BLE001 -- the headline line must still come out
            out["config4"] = {"error": str(e)}
    if cpu is not None:
        out["cpu_baseline"] = cpu
    print(json.dumps(out), flush=True)
    if dist:
        dist.destroy_process_group()


def real_features(ssw, model, torch, steps=50):
    """The scoring step on features of a real recording: the 13-dim cepstra of the reference's
    goforward.wav (tests/golden/goforward_mfcc.npy, made by tests/golden/make_mfcc.py) through
    ssw_feat_batch (batch CMN + deltas on the GPU), tiled to 16 utterances x 256 frames.  The
    share of pairs that needs the exact pass depends on the data; synthetic features sit close
    to the Gaussian means."""
    path = os.path.join(ROOT, "tests", "golden", "goforward_mfcc.npy")
    if not os.path.exists(path):
        return None
    cep = np.load(path).astype(np.float32)
    feat = model.feat_batch(cep)                       # [n][39], one utterance
    reps = -(-N_UTTS * UTT_FRAMES // feat.shape[0])
    tiled = np.tile(feat, (reps, 1))[:N_UTTS * UTT_FRAMES].copy()
    off = (np.arange(N_UTTS + 1) * UTT_FRAMES).astype(np.int32)
    st = ScoreStep(torch, model, tiled, off)
    spin_up(torch, st, 0.3)
    e, e_dev = timed_steps(torch, None, "nccl", st, 5, steps)
    k = np.array([e_dev / steps])
    flagged, pairs = model.last_stats()
    return {"workload": f"{len(cep)} frames of goforward.wav (cepstra -> ssw_feat_batch), tiled to "
                        f"{N_UTTS} x {UTT_FRAMES} frames",
            "frames_per_s": st.n_frames * steps / e, "ms_per_step": e / steps * 1e3,
            "kernel_ms": float(k.sum()), "exact_pass_share": flagged / max(pairs, 1)}


if __name__ == "__main__":
    main()
