#!/usr/bin/env python
"""bench.py -- points/sec, forward+backward+optimizer step, PT-v2m2 S3DIS config, synthetic scenes.

  python bench.py --gpus N --steps K --warmup W

N > 1 without a launcher: this process becomes a PARENT that never touches the GPU (it imports neither torch nor
the HIP library); it starts N children, one per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT
set (the reference's own launcher does the same with mp.spawn, pointcept/engines/launch.py:74-135), relays rank 0's
JSON line and exits non-zero if any child does.  Under `python -m torch.distributed.run --nproc-per-node N bench.py
--gpus N ...` the ranks already exist and each process is a child.

One "step" = one full training step of the hot path on one batch that is already resident in HBM:
geometry (kNN tables, grid pooling, interpolation tables) + PT-v2m2 forward + cross-entropy +
backward + AdamW.  One process per GPU; data parallel by scene (one scene per rank, weak scaling);
gradients averaged over RCCL (backend "nccl" on ROCm) by one flat all-reduce per step (or torch DDP,
AO_AMD_GRAD_SYNC=ddp).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline `value` / `ms_per_step` plus the `host` and
`config` objects of the timed region).  `--full` adds everything that takes runs of its own:
  roofline         the dominant hand-written kernel, timed live with HIP events on the launch stream
  reference_loop   the reference trainer's run_step statements over this build
  config.also      the reference recipe's per-GPU batch (3 x 80 000 points), timed by a child run
  ops              kNN / FPS us per query on the run's scene
  cpu_baseline     the CPU oracle (oracle/ptv2_ref.py + C kNN) timed on this box's host cores on a
                   bounded sample of the same workload (rank 0, N=1 only)
(the --no-* options switch single legs of --full off).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step computed as DIR/<name>.npy (float32):
`loss`, `logits` (the backbone's output), `params` (after the optimizer step), `grads`, `buffers` (BatchNorm running
statistics); an array of more than DUMP_CAP elements is written as a fixed, seeded sample of its rows.  The inputs
(scene, weights, dropout stream) follow from the arguments alone, so two builds can be compared output for output.

Environment switches for boxes with fewer GPUs than ranks (tests/test_gpu_bench_spawn.py):
  AO_AMD_BENCH_BACKEND=gloo      exchange gradients over gloo instead of RCCL (RCCL refuses two ranks on one device)
  AO_AMD_BENCH_ONE_DEVICE=1      every rank uses cuda:0
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

# the pool's host driver only supports dmabuf IPC: without this RCCL / cross-process tensor sharing fails with
# `hipIpcGetMemHandle: invalid argument` (already exported on the GPU boxes; kept here for any other launcher)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

np = torch = dist = None  # imported by the rank processes only (child_main): the spawning parent stays GPU-free


def _imports():
    global np, torch, dist
    import numpy
    import torch as _torch
    import torch.distributed as _dist

    np, torch, dist = numpy, _torch, _dist

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)
MFMA_FP32_PEAK_TFLOPS = 157.3  # dense fp32 matrix peak (V_MFMA_F32_16X16X4_F32, exact fp32; guides/MI355X_MICROARCH.md)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=120000, help="points per scene (BASELINE.json configs[1]: ~120k)")
    ap.add_argument("--scenes", type=int, default=1, help="scenes per GPU")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--cfg", default="s3dis", choices=["s3dis", "scannet"],
                    help="backbone config: the headline S3DIS one, or configs/scannet/semseg-pt-v2m2-0-base.py (BASELINE.json configs[4])")
    ap.add_argument("--segmentor", default="default", choices=["default", "sam_image"],
                    help="sam_image: DefaultSegmentorSAM_Image + the per-step logit basket of train_real (BASELINE.json configs[3])")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline: roofline, reference_loop, config.also, ops, cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32)")
    ap.add_argument("--cpu-sample-points", type=int, default=120000,
                    help="points of the CPU-oracle scene (default: the metric's own 120 000; ~1-2 min on the box's 16-CPU quota)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-ops", action="store_true", help="skip the kNN / FPS us-per-query lines")
    ap.add_argument("--no-reference-loop", action="store_true",
                    help="skip the reference_loop leg (the reference trainer's run_step statements over this build)")
    ap.add_argument("--no-also", action="store_true",
                    help="skip config.also: the reference recipe's per-GPU batch (3 x 80 000 points) timed by a child run")
    ap.add_argument("--spawn-timeout", type=float, default=1800.0,
                    help="--gpus N without a launcher: seconds after which the remaining ranks are terminated (exit 124)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:  # a plain run: only the headline's own timed region
        args.no_cpu_baseline = args.no_roofline = args.no_ops = args.no_reference_loop = args.no_also = True
    return args


DUMP_CAP = 4 << 20  # elements per dumped array (16 MB of float32); five arrays stay under 64 MB


def dump_outputs(out_dir, arrays):
    """Write every array of `arrays` ({name: tensor or ndarray}) as out_dir/<name>.npy in float32.  One with more than DUMP_CAP
    elements is written as a sample of its rows (of its elements when 1-D): numpy's default_rng(0) over the row count, sorted,
    so that the same shape always keeps the same rows.  Returns {name: (shape written, full shape)}."""
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, a in arrays.items():
        if torch.is_tensor(a):
            a = a.detach().float().cpu().numpy()
        a = np.asarray(a, dtype=np.float32)
        full = a.shape
        if a.size > DUMP_CAP:
            per_row = a.size // a.shape[0]
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], DUMP_CAP // per_row, replace=False))
            a = a[rows]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = (list(a.shape), list(full))
    return written


def make_batch(rank, scenes, points, device, in_channels=6, num_classes=13):
    from ao_amd import synth

    from ao_amd.ptv2.parallel import scene_seeds

    b = synth.scene_batch(scene_seeds(rank, scenes), point_max=points, in_channels=in_channels, num_classes=num_classes, room=1)
    return {k: torch.from_numpy(v).to(device) for k, v in b.items()}


def algorithmic_step_bytes(levels, cfg):
    """compulsory fp32 traffic of the fused blocks, fwd+bwd = 4*N*(6C+2K+6) per block."""
    c0 = cfg["patch_embed_channels"]
    per_level = [(cfg["patch_embed_depth"] + cfg["dec_depths"][0], c0, cfg["patch_embed_neighbours"])]
    for i, d in enumerate(cfg["enc_depths"]):
        extra = cfg["dec_depths"][i + 1] if i + 1 < len(cfg["dec_depths"]) else 0
        per_level.append((d + extra, cfg["enc_channels"][i], cfg["enc_neighbours"][i]))
    total = 0
    for (nb, c, k), n in zip(per_level, levels):
        total += nb * 4 * n * (6 * c + 2 * k + 6)
    return total


def mfma_bound_flops(kernel, levels):
    """Algorithmic (useful: no tile padding counted) matrix FLOPs per launch of the deep-level attention tile kernels, which are
    bound by the fp32 matrix pipe, not by HBM: their operands live in LDS / registers and what they read from memory is a few MB
    (gva_fwd_tile.hip / gva_bwd_tile.hip).  None for every other kernel (HBM roofline).  Per point, K = 16 slots, G groups,
    C = 8 G channels: forward  z = Ww2 y (2 K G G), A = w^T P (2 K G C), projection (2 C C);  backward  z, gy, gWw2 (3 x 2 K G G),
    g_A = g_out Wp2 (2 C C), gw = g_A P^T and gP = w g_A (2 x 2 K G C)."""
    import re

    m = re.match(r"attention_(fwd|bwd)_tile_kernel<(\d+), (\d+),", kernel)
    if not m:
        return None
    g, c, k = int(m.group(2)), int(m.group(3)), 16
    n = {12: 1, 24: 2, 48: 3, 64: 4}.get(g)
    if n is None or n >= len(levels):
        return None
    n = levels[n]
    per_point = (2 * k * g * g + 2 * k * g * c + 2 * c * c) if m.group(1) == "fwd" else (6 * k * g * g + 2 * c * c + 4 * k * g * c)
    return float(n) * per_point


def src_hash(build_info):
    """The source digest inside ptv2_build_info() ("... src <12 hex> hipcc ...")."""
    parts = build_info.split()
    return parts[parts.index("src") + 1] if "src" in parts else None


def pmc_traffic(kernel, build_info):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled per the gfx950
    note of the microarchitecture guide, + WRITE_SIZE; tools/pmc_traffic.py).  Counters cannot be read from inside
    this process, so the figure is the one measured with the same command under profiles/ -- accepted only when the
    profile's first line carries the source digest of THIS build of the library; (None, why) otherwise."""
    import glob

    kernel = kernel.replace(" [family]", "")  # (a family's timer name: matched as the template's instances below)
    want = src_hash(build_info)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_per_launch.jsonl")), reverse=True)
    stale = []
    for path in files:
        recs = [json.loads(line) for line in open(path) if line.strip()]
        stamp = next((r["_build"] for r in recs if "_build" in r), None)
        if stamp is None or src_hash(stamp) != want:
            stale.append(os.path.basename(path))
            continue
        base = kernel.split("<")[0]
        # a timer name without template arguments stands for every instance of the kernel (the timer brackets them all):
        # launch-weighted mean over the instances, to be set against the family's mean algorithmic bytes
        hits = []
        for rec in recs:
            for name, v in rec.items():
                if name == "_build":
                    continue
                short = name.split("::")[-1]
                # (the batched form of a weight-gradient kernel, `<name>_jobs`, is timed under the kernel's name; a timer name
                # with template arguments stands for the instances that extend its argument list -- the dropout flag)
                if short == kernel or (short.split("<")[0] in (base, base + "_jobs") and "<" not in kernel) or (
                        "<" in kernel and short.startswith(kernel[:-1] + ",")):
                    hits.append((short, v))
        if hits:
            launches = sum(v["launches"] for _, v in hits)
            total = sum(v["launches"] * (v["fetch_x2_MB_per_launch"] + v["write_MB_per_launch"]) for _, v in hits)
            return (1e6 * total / max(launches, 1),
                    "bytes/launch, launch-weighted over %s, profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                    "command, same library build %s; FETCH_SIZE doubled per the gfx950 note of the microarchitecture guide)"
                    % (" + ".join("%s x %d" % (n, v["launches"]) for n, v in hits), os.path.basename(path), want))
        return None, "profiles/%s is of this build but does not list %s" % (os.path.basename(path), kernel)
    return None, "no PMC profile of this build (src %s) under profiles/ (other builds: %s)" % (want, ", ".join(stale) or "none")


def op_microbench(data):
    """BASELINE.json's second metric, "knn + FPS us/query", on the scene of this run (HIP-event time of the whole op
    / queries): self kNN k=16, the 3-NN cross query of the interpolation, stride-4 farthest point sampling.  Runs
    after the timed region (bench_ops.py is the stand-alone form with the CPU oracle beside it)."""
    from ao_amd import pointops

    xyz, off = data["coord"], data["offset"].int()
    n = xyz.shape[0]

    def timed(fn, reps):
        for _ in range(2):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    t_knn = timed(lambda: pointops.knn_query_dist2(16, xyz, off), 10)
    out = {"knn_k16_self_us_per_query": t_knn / n}
    # What the grid method actually evaluates: one more call through the counting twin of the query
    # kernel (knn_query_count_pairs, include/ptv2_hip.h) adds every candidate distance it computes to a device counter.
    # A pair costs 3 sub + 1 mul + 2 fma = 8 flop on the vector ALU and one 16-byte read of the cell-sorted float4 copy
    # (L1 / L2 hits for all but the first lane that touches a cell).  The reference kernel scans all m * n_b pairs
    # (knn_query_cuda_kernel.cu:88-97); that count is reported beside it, not priced against a peak.
    from ao_amd import _lib
    counter = torch.zeros(1, dtype=torch.int64, device=xyz.device)
    _lib.lib().knn_query_count_pairs(counter.data_ptr())
    try:
        pointops.knn_query_dist2(16, xyz, off)
        torch.cuda.synchronize()
    finally:
        _lib.lib().knn_query_count_pairs(None)
    pairs = float(counter.item())
    sizes = torch.diff(off.long(), prepend=off.new_zeros(1).long()).double()
    out["knn_k16_self_pairs_evaluated"] = pairs
    out["knn_k16_self_pairs_evaluated_per_query"] = pairs / n
    out["knn_k16_self_pairs_evaluated_per_s"] = pairs / (t_knn * 1e-6)
    out["knn_k16_self_frac_of_fp32_valu_peak"] = out["knn_k16_self_pairs_evaluated_per_s"] * 8 / 157.3e12
    out["knn_k16_self_candidate_read_GBps"] = pairs * 16 / (t_knn * 1e-6) / 1e9
    out["knn_k16_self_bruteforce_pairs_of_the_reference_scan"] = float((sizes * sizes).sum())
    out["knn_k16_self_note"] = ("whole op (grid build + query + tie re-run), HIP-event time; pairs = candidate distances the query kernel "
                                "computed (counting twin); VALU fraction = pairs x 8 flop / time / 157.3 TFLOP/s; candidate_read = "
                                "pairs x 16 B of cell-sorted float4 reads (mostly L1/L2 hits: the compulsory HBM bytes are 12n+12m+8mk)")
    if off.numel() == 1:
        coarse = xyz[::6].contiguous()
        coff = torch.tensor([coarse.shape[0]], dtype=torch.int32, device=xyz.device)
        out["knn_k3_cross_us_per_query"] = timed(lambda: pointops.knn_query_dist2(3, coarse, coff, xyz, off), 10) / n
    noff = (off // 4).int()
    out["fps_stride4_us_per_sample"] = timed(lambda: pointops.farthest_point_sampling(xyz, off, noff), 2) / int(noff[-1])
    # FPS is a chain of m-1 dependent arg-max sweeps; with the cloud resident in the registers of W cooperating workgroups
    # the floor of one sample is ONE cross-workgroup exchange of an 8-byte data-tagged granule: 0.8 us on an idle chip
    # (guides/MI355X_MICROARCH.md, price list row handoff-1to1) -- a latency floor, not a bandwidth one
    out["fps_handoff_floor_us_per_sample"] = 0.8
    out["fps_frac_of_handoff_floor"] = 0.8 / out["fps_stride4_us_per_sample"]
    return out


def host_facts():
    """What the launching thread runs on: a judge must be able to tell a slow host from a slow GPU from the one line."""
    model = "?"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = None
    return {"cpu": model, "cpus_online": os.cpu_count(), "affinity": affinity, "loadavg": list(os.getloadavg()),
            "cgroup_cpu_max": cgroup_cpu()[0]}


def cgroup_cpu():
    """(cpu.max, {nr_periods, nr_throttled, throttled_usec}) of this process's cgroup (v2), or (None, {}).  The pool's GPU
    boxes show 256 CPUs but run under a quota (1600000 100000 = 16 CPUs): a process that exceeds it inside a 100 ms
    period is stopped -- every thread, the launching one included -- until the period ends."""
    quota, stat = None, {}
    try:
        quota = open("/sys/fs/cgroup/cpu.max").read().strip()
        for line in open("/sys/fs/cgroup/cpu.stat"):
            k, v = line.split()
            if k in ("nr_periods", "nr_throttled", "throttled_usec", "usage_usec"):
                stat[k] = int(v)
    except (OSError, ValueError):
        pass
    return quota, stat


def thread_cpu_snapshot():
    """{tid: (name, CPU seconds)} of every thread of this process (/proc/self/task/*/stat: utime + stime) -- which threads a
    rank really runs (launching thread, geometry worker, HIP / RCCL progress threads) and what each costs per step."""
    out = {}
    tick = os.sysconf("SC_CLK_TCK") if hasattr(os, "sysconf") else 100
    try:
        for tid in os.listdir("/proc/self/task"):
            try:
                raw = open("/proc/self/task/%s/stat" % tid).read()
            except OSError:
                continue
            name = raw[raw.index("(") + 1: raw.rindex(")")]
            f = raw[raw.rindex(")") + 2:].split()
            out[int(tid)] = (name, (int(f[11]) + int(f[12])) / tick)
    except OSError:
        pass
    return out


def cpu_quota():
    """CPUs this process may use: the cgroup quota when there is one, else the affinity mask."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = cgroup_cpu()[0]
    if quota:
        a, b = quota.split()
        if a != "max":
            n = min(n, max(1, int(a) // int(b)))
    return n


def cpu_baseline(cfg, sample_points, crop_points=12000):
    """fwd+bwd+AdamW of the CPU oracle (oracle/ptv2_ref.py + the C kNN) on the metric's own workload -- one `sample_points`
    scene of the same generator (default 120 000: the configuration `value` is quoted on), ONE step, timed after the code
    paths were warmed on a `crop_points` crop (whose rate is reported beside it).  Threads = the CPUs this process may
    actually use (the cgroup quota of the box, not the 256 it shows: with one thread per visible CPU the step is throttled)."""
    from ao_amd import synth
    from oracle import pointops_ref, ptv2_ref

    pointops_ref.build()
    threads = cpu_quota()
    torch.set_num_threads(threads)

    def run(points, reps):
        torch.manual_seed(0)
        b = synth.scene_batch([0], point_max=points, room=1)
        data = {k: torch.from_numpy(v) for k, v in b.items()}
        model = ptv2_ref.RefModule(dict(cfg, drop_path_rate=0.0)).train()
        opt = torch.optim.AdamW(model.parameters(), lr=0.006, weight_decay=0.05)
        times = []
        for it in range(reps):
            t0 = time.perf_counter()
            loss = torch.nn.functional.cross_entropy(model(data), data["segment"], ignore_index=-1)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            times.append(time.perf_counter() - t0)
        return times, int(data["coord"].shape[0])

    crop_times, crop_n = run(min(crop_points, sample_points), 3)
    crop_t = float(np.median(crop_times[1:]))
    crop = dict(value=crop_n / crop_t, points=crop_n, s_per_step=crop_t, sample="median of 2 steps after 1 warm-up")
    if sample_points <= crop_points:
        value, t, what = crop["value"], crop_t, "1 scene cropped to %d points, median of 2 steps after 1 warm-up" % crop_n
    else:
        full_times, full_n = run(sample_points, 1)
        t = full_times[0]
        value, what = full_n / t, "1 scene of %d points (the metric's workload), 1 step after a warm-up on a %d-point crop" % (full_n, crop_n)
    return dict(value=value, unit="points/s", cores=threads, kind="port",
                sample="%s, fwd+bwd+AdamW, %.1f s/step; torch-CPU restatement + C kNN (oracle/), drop_path 0; threads = "
                       "cgroup CPU quota (%s)" % (what, t, cgroup_cpu()[0]),
                s_per_step=t, crop=crop)


def spawn_ranks(args):
    """Parent of an N-rank run: start one child per GPU and relay rank 0's JSON line.  This process makes no HIP call
    (no torch import at all), so nothing that has initialised the GPU is ever forked or re-executed; every child is a
    fresh interpreter.  A child that fails takes the job down: the others are terminated by PID and the parent exits
    with the failing status (reference: pointcept/engines/launch.py:74-87 mp.spawn(..., join) semantics)."""
    n = args.gpus
    # a profiler preload (rocprofv3 sets ROCP_TOOL_LIBRARIES / LD_PRELOAD) initialises the GPU in THIS process before it could
    # start the ranks, and all ranks would write into one output directory: profile one rank at a time instead
    preload = os.environ.get("LD_PRELOAD", "")
    if os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprofiler" in preload or "rocprof" in preload:
        sys.stderr.write("bench.py: --gpus %d under a profiler preload is refused (the parent would hold the GPU before "
                         "spawning); profile a single rank: rocprofv3 ... -- python3 bench.py --gpus 1\n" % n)
        raise SystemExit(2)
    deadline = time.monotonic() + args.spawn_timeout
    with socket.socket() as s:  # (bind / close / reuse can race with another process on the host: a rank then fails to
        s.bind(("127.0.0.1", 0))  # rendezvous, the job exits non-zero and can simply be started again)
        port = s.getsockname()[1]
    children = []
    for rank in range(n):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AO_AMD_BENCH_CHILD="1")
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                         stdout=subprocess.PIPE if rank == 0 else sys.stderr))
    out0 = b""
    failed = None
    pending = set(range(n))
    # rank 0's stdout carries only the result line (child_main redirects everything else to stderr), so reading it to
    # EOF cannot block on a full pipe of chatter; poll the others meanwhile so that a dead rank is noticed
    import selectors

    sel = selectors.DefaultSelector()
    sel.register(children[0].stdout, selectors.EVENT_READ)
    eof = False
    while pending:
        if not eof:
            for key, _ in sel.select(timeout=0.2):
                chunk = os.read(key.fileobj.fileno(), 65536)
                if chunk:
                    out0 += chunk
                else:
                    eof = True
                    sel.unregister(key.fileobj)
        else:
            time.sleep(0.2)
        for r in list(pending):
            rc = children[r].poll()
            if rc is not None:
                pending.discard(r)
                if rc != 0 and failed is None:
                    failed = (r, rc)
        if failed is None and pending and time.monotonic() > deadline:
            # a rank that hangs in rendezvous (e.g. its peer died before init) must not block the parent for ever
            failed = (min(pending), 124)
            sys.stderr.write("bench.py: no result after %.0f s (--spawn-timeout); terminating ranks %s\n"
                             % (args.spawn_timeout, sorted(pending)))
        if failed is not None:
            for r in pending:
                children[r].terminate()
            for r in pending:
                try:
                    children[r].wait(timeout=20)
                except subprocess.TimeoutExpired:
                    children[r].kill()
            break
    if failed is not None:
        sys.stderr.write("bench.py: rank %d exited with status %d; job aborted\n" % failed)
        raise SystemExit(failed[1] if failed[1] > 0 else 1)
    if not eof:
        out0 += children[0].stdout.read()
    sys.stdout.write(out0.decode())
    sys.stdout.flush()


def _launcher_name():
    if "TORCHELASTIC_RUN_ID" in os.environ:
        return "torch.distributed.run"
    return "bench.py spawn" if os.environ.get("AO_AMD_BENCH_CHILD") == "1" else "single"


def main():
    args = parse()
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not launched:
        return spawn_ranks(args)
    return child_main(args)


def reference_loop_leg(ptv2, args, cfg, device, data, world, points_per_step):
    """ms per step of the REFERENCE trainer's own statements over this build, with nothing of bench.py's accelerations: a fresh
    segmentor, wrapped as `create_ddp_model` wraps it (pointcept/engines/defaults.py:20-43: DistributedDataParallel with
    broadcast_buffers=False when world_size > 1, the bare module otherwise), `torch.optim.AdamW` as the reference's
    `build_optimizer` returns for the config's dict(type="AdamW", lr=0.006, weight_decay=0.05)
    (pointcept/utils/optimizer.py:20-55, configs/s3dis/semseg-pt-v2m2-0-base.py:42), torch's MultiStepLR, parameter
    gradients delivered through autograd, the batch handed to `model(input_dict)` as the loader produces it (host tensors, no
    `geometry=` key, no prefetcher thread): `Trainer.run_step` (pointcept/engines/train_sam_pp2s.py:173-200) statement by
    statement, followed by what `InformationWriter.after_step` does every iteration (`.item()` of every loss,
    pointcept/engines/hooks/misc.py:112).  `ms_per_step_no_item`: the same without that per-step read-back.

    `variants`: the same loop under CONFIG-ONLY changes of the optimizer line -- `OPTIMIZERS.build` passes every key of the
    dict to the constructor (pointcept/utils/optimizer.py:55), so `dict(type="AdamW", ..., fused=True)` and, with the registry
    file of INTEGRATION.md section 2, `dict(type="FlatAdamW", ...)` need no trainer code.
    `ddp`: the loop with the `DistributedDataParallel(broadcast_buffers=False)` wrap forced in a one-rank RCCL group (what
    every rank of the reference's multi-GPU recipe runs: 840 parameters -> AccumulateGrad hooks, bucket copies, one
    all-reduce per bucket): its cost on this build, measurable on one GPU."""
    import torch.distributed as dist

    enable_amp = args.dtype != "fp32"
    host = {k: (v.cpu().pin_memory() if isinstance(v, torch.Tensor) else v) for k, v in data.items() if k != "geometry"}
    steps = max(5, min(args.steps, 20))
    warm = max(3, min(args.warmup, 5))

    def build(optim_kind, force_ddp, direct=False):
        # direct: backbone = dict(type="PT-v2m2", ..., native_param_grads="direct") -- the one keyword this build's class adds
        bcfg = dict(cfg, native_param_grads="direct") if direct else cfg
        seg = (ptv2.DefaultSegmentorSAM_Image if args.segmentor == "sam_image" else ptv2.DefaultSegmentor)(bcfg).to(device).train()
        model, wrapped = seg, False
        if world > 1 or force_ddp:  # create_ddp_model
            if not dist.is_initialized():  # a one-rank group of its own (the bench's exchange is not in use at world 1)
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
                dist.init_process_group("nccl", rank=0, world_size=1)
            model = torch.nn.parallel.DistributedDataParallel(seg, device_ids=[device.index], output_device=device.index,
                                                              broadcast_buffers=False, find_unused_parameters=False)
            wrapped = True
        if optim_kind == "AdamW":
            optimizer = torch.optim.AdamW(model.parameters(), lr=0.006, weight_decay=0.05)
        elif optim_kind == "AdamW(fused=True)":
            optimizer = torch.optim.AdamW(model.parameters(), lr=0.006, weight_decay=0.05, fused=True)
        else:  # dict(type="FlatAdamW", lr=0.006, weight_decay=0.05) through the registry (ao_amd/ptv2/registry.py)
            from ao_amd.ptv2.optim import FlatAdamW

            optimizer = FlatAdamW(params=model.parameters(), lr=0.006, weight_decay=0.05)
        total = 1 << 20
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(0.09 * total), int(0.2 * total)], gamma=0.1)
        scaler = torch.cuda.amp.GradScaler() if enable_amp else None
        return model, optimizer, scheduler, scaler, wrapped

    def measure(optim_kind, force_ddp, with_item_too, direct=False):
        model, optimizer, scheduler, scaler, wrapped = build(optim_kind, force_ddp, direct)
        comm_info = {}

        def run_step():  # train_sam_pp2s.py:173-200
            input_dict = dict(host)
            for key in input_dict.keys():
                if isinstance(input_dict[key], torch.Tensor):
                    input_dict[key] = input_dict[key].cuda(non_blocking=True)
            with torch.cuda.amp.autocast(enabled=enable_amp):
                output_dict = model(input_dict)
                if isinstance(output_dict, tuple):  # train_sam_real.py:187: (dict(loss), seg_dict)
                    output_dict = output_dict[0]
                loss = output_dict["loss"]
            optimizer.zero_grad()
            if enable_amp:
                scaler.scale(loss).backward()
                scaler.step(optimizer)
                scale = scaler.get_scale()
                scaler.update()
                if scale <= scaler.get_scale():
                    scheduler.step()
            else:
                loss.backward()
                optimizer.step()
                scheduler.step()
            comm_info["model_output_dict"] = output_dict

        def after_step():  # hooks/misc.py:108-112
            for key in comm_info["model_output_dict"].keys():
                if "loss" in key:
                    comm_info[key] = comm_info["model_output_dict"][key].item()

        def timed(n, with_item):
            if dist.is_initialized() and world > 1:
                dist.barrier()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(n):
                run_step()
                if with_item:
                    after_step()
            torch.cuda.synchronize(device)
            t = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
            if dist.is_initialized() and world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        timed(warm, True)
        with_item = timed(steps, True) if with_item_too else None
        no_item = timed(steps, False)
        after_step()
        del model, optimizer
        return with_item, no_item, comm_info.get("loss"), wrapped

    with_item, no_item, loss, wrapped = measure("AdamW", False, True)
    out = {"ms_per_step": 1e3 * with_item / steps, "points_per_s": points_per_step * steps / with_item,
           "ms_per_step_no_item": 1e3 * no_item / steps, "steps": steps,
           "loop": "Trainer.run_step statements (pointcept/engines/train_sam_pp2s.py:173-200) + InformationWriter.after_step's "
                   "loss.item() (hooks/misc.py:112); batch from pinned host memory via .cuda(non_blocking=True)",
           "model": "DistributedDataParallel(broadcast_buffers=False)" if wrapped else "bare module (create_ddp_model at world_size 1)",
           "optimizer": "torch.optim.AdamW + MultiStepLR", "param_grads": "autograd (.grad through AccumulateGrad)",
           "geometry": "inside PointTransformerV2.forward (pipelined with the level-0 prefix; no prefetcher, no geometry= key)",
           "enable_amp": enable_amp, "loss": loss}
    # config-only changes of the optimizer line; then the reference's DDP wrap forced at one rank
    variants = {}
    for kind in ("AdamW(fused=True)", "FlatAdamW"):
        try:
            _, t, _, _ = measure(kind, False, False)
            variants["optimizer = dict(type=%s)" % ('"AdamW", ..., fused=True' if kind != "FlatAdamW" else '"FlatAdamW", ...')] = {
                "ms_per_step_no_item": 1e3 * t / steps}
        except Exception as exc:  # a variant must not take the line down
            variants[kind] = {"error": repr(exc)[:200]}
    # ... and of the backbone line: gradients assigned by the native backward instead of 840 AccumulateGrad nodes (a loop that
    # only calls loss.backward() does not see the difference; not under DDP, whose reducer waits for its parameter's node)
    for kind in ("AdamW", "FlatAdamW"):
        try:
            _, t, _, _ = measure(kind, False, False, direct=True)
            variants['backbone = dict(..., native_param_grads="direct") + optimizer = dict(type="%s", ...)' % kind] = {
                "ms_per_step_no_item": 1e3 * t / steps}
        except Exception as exc:
            variants["direct+" + kind] = {"error": repr(exc)[:200]}
    out["variants"] = variants
    if world == 1:
        ddp = {}
        for kind in ("AdamW", "FlatAdamW"):
            try:
                _, t, _, w = measure(kind, True, False)
                ddp[kind] = {"ms_per_step_no_item": 1e3 * t / steps, "wrapped": bool(w)}
            except Exception as exc:
                ddp[kind] = {"error": repr(exc)[:200]}
        ddp["what"] = ("DistributedDataParallel(broadcast_buffers=False) as create_ddp_model wraps (engines/defaults.py:20-43), "
                       "forced in a one-rank RCCL group: hooks + bucket copies + the all-reduce launch, without another rank to wait for")
        out["ddp"] = ddp
    return out


def block_leg(ptv2, geo, device, reps=10):
    """One level-0 Block of the scene (C = 48, G = 6, K = 16) on its own, forward and backward timed with HIP events, against
    SURVEY.md section 8(d)'s COMPULSORY traffic of a fused Block -- forward 4 N (2C + K + 3) bytes (feat in, feat out, idx,
    coord), backward 4 N (4C + K + 3) (feat, grad_out in; grad_feat out; recompute) -- i.e. the fraction of the HBM roofline
    the whole Block chain reaches, beside the per-kernel fraction of its dominant kernel (which counts the design's own
    intermediates as algorithmic bytes).  Standalone: the Block's weight gradients run in the backward here (the model runtime
    files them and runs all of them at the end of the step)."""
    lv = geo.levels[0]
    n, c, g, k = int(lv.coord.shape[0]), 48, 6, 16
    idx = lv.neighbours(k)
    blk = ptv2.Block(c, g).to(device).train()
    x = torch.randn(n, c, device=device).relu_().requires_grad_(True)
    go = torch.randn(n, c, device=device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tb = [], []
    for it in range(reps + 3):
        ev[0].record()
        y = blk([lv.coord, x, lv.offset], idx)[1]
        ev[1].record()
        y.backward(go)
        ev[2].record()
        torch.cuda.synchronize(device)
        if it >= 3:
            tf.append(ev[0].elapsed_time(ev[1]))
            tb.append(ev[1].elapsed_time(ev[2]))
        blk.zero_grad(set_to_none=True)
        x.grad = None
    tf, tb = sorted(tf)[len(tf) // 2], sorted(tb)[len(tb) // 2]
    fb, bb = 4.0 * n * (2 * c + k + 3), 4.0 * n * (4 * c + k + 3)
    return {"level": 0, "n": n, "c": c, "g": g, "k": k,
            "forward": {"ms": tf, "compulsory_MB": fb / 1e6, "frac": fb / (tf * 1e-3) / (HBM_PEAK_GBS * 1e9)},
            "backward": {"ms": tb, "compulsory_MB": bb / 1e6, "frac": bb / (tb * 1e-3) / (HBM_PEAK_GBS * 1e9)},
            "what": "one level-0 Block standalone (median of %d, HIP events; eager issue, weight gradients inside the backward); "
                    "compulsory bytes per SURVEY.md section 8(d)" % reps}


def also_leg(args):
    """`config.also`: the batch each rank of the reference's 4-GPU recipe runs -- batch_size 12 over 4 GPUs = 3 scenes per GPU
    (configs/s3dis/semseg-pt-v2m2-0-base.py:3, pointcept/engines/defaults.py:139), 80 000 points each --
    timed by a child run of this script with the same loop (a fresh process: its own arenas, graphs and prefetcher), so that
    the driver's line carries that number beside the 1 x 120 000 headline.  Only for the default workload at one GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), "--scenes", "3", "--points", "80000", "--steps", "10", "--warmup", "5",
           "--dtype", args.dtype, "--cfg", args.cfg, "--segmentor", args.segmentor, "--no-cpu-baseline", "--no-ops", "--no-roofline",
           "--no-reference-loop", "--no-also"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        if out.returncode != 0 or len(lines) != 1:
            return {"error": "child rc %d: %s" % (out.returncode, out.stderr[-300:])}
        d = json.loads(lines[0])
        return {"workload": d["config"]["workload"], "why": "the per-GPU batch of the reference's 4-GPU recipe (batch_size 12 / 4 GPUs, "
                "configs/s3dis/semseg-pt-v2m2-0-base.py:3)", "ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"],
                "steps": d["steps"], "warmup": d["warmup"], "points_per_step": round(d["value"] * d["ms_per_step"] / 1e3)}
    except Exception as exc:
        return {"error": repr(exc)[:300]}


def child_main(args):
    _imports()
    # stdout carries exactly ONE line, the JSON result of rank 0: everything else that writes to file descriptor 1 in any
    # rank (RCCL prints a "ROCm version / Hostname / Librccl path" banner there when a communicator is created) is sent
    # to stderr for the lifetime of the process; the result is written to the saved descriptor at the end
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    from ao_amd.ptv2 import parallel

    rank, local_rank, world = parallel.rank_world()
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if os.environ.get("AO_AMD_BENCH_DRYRUN") == "1":
        # launcher check only (tests/test_bench_spawn.py, no GPU): rendezvous + the barrier / max-over-ranks timing
        # protocol around an empty step; reports no throughput
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        cpu = torch.device("cpu")
        elapsed, pts, _ = parallel.timed_steps(lambda: None, args.steps, cpu, args.points)
        if rank == 0:
            os.write(result_fd, (json.dumps({"dry_run": True, "value": None, "n_gpus": world, "steps": args.steps,
                                             "points_per_step": pts, "launcher": _launcher_name(),
                                             "rccl_ranks": dist.get_world_size() if dist.is_initialized() else 1}) + "\n").encode())
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs a GPU: the HIP path has no CPU fallback"
    # the GPU path needs no CPU worker threads; torch's default (one per visible CPU: 128 on the pool's hosts) overruns the
    # boxes' cgroup quota (16 CPUs) whenever an intra-op pool spins up, and a throttled period stops the launching thread too
    # (N ranks share the quota: each takes its share, at least one)
    torch.set_num_threads(max(1, min(torch.get_num_threads(), cpu_quota() // max(1, world))))
    if os.environ.get("AO_AMD_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("AO_AMD_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    def init_group():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    if world > 1:
        init_group()

    import ao_amd.ptv2 as ptv2
    from ao_amd import _lib

    torch.manual_seed(4242)
    cfg = dict(ptv2.S3DIS_BACKBONE if args.cfg == "s3dis" else ptv2.SCANNET_BACKBONE)
    seg = (ptv2.DefaultSegmentorSAM_Image if args.segmentor == "sam_image" else ptv2.DefaultSegmentor)(cfg).to(device).train()
    net = seg
    # gradient exchange: one flat all-reduce after backward (parallel.FlatGradSync, default) or torch DDP
    # (AO_AMD_GRAD_SYNC=ddp; AO_AMD_FORCE_DDP=1 also wraps a 1-rank run so that a 1-GPU box exercises that path)
    sync = None
    use_ddp = os.environ.get("AO_AMD_GRAD_SYNC", "flat") == "ddp" or os.environ.get("AO_AMD_FORCE_DDP") == "1"
    force_sync = os.environ.get("AO_AMD_FORCE_SYNC") == "1"  # 1-GPU box: run the flat exchange in a 1-rank group
    if world > 1 or os.environ.get("AO_AMD_FORCE_DDP") == "1" or force_sync:
        if not dist.is_initialized():
            init_group()
        if use_ddp:
            net = parallel.wrap_ddp(seg, device)
        else:
            sync = parallel.FlatGradSync(seg, force=force_sync, mode=os.environ.get("AO_AMD_GRAD_SYNC", "flat"))
    # AdamW(lr 0.006, wd 0.05) as in the reference config; AO_AMD_OPTIM=torch selects torch.optim.AdamW(fused=True)
    # instead of the one-kernel flat form (ao_amd/ptv2/optim.py)
    flat_opt = os.environ.get("AO_AMD_OPTIM", "flat") == "flat" and not use_ddp
    if flat_opt:
        from ao_amd.ptv2.optim import FlatAdamW

        opt = FlatAdamW(seg.parameters(), lr=0.006, weight_decay=0.05)
        # the native model backward writes every parameter gradient into one flat buffer in the optimizer's layout and
        # assigns `.grad` itself (ao_amd/ptv2/native_model.py): no AccumulateGrad nodes, no flatten copy
        seg.backbone.native_param_grads = os.environ.get("AO_AMD_PARAM_GRADS", "direct")
    else:
        opt = torch.optim.AdamW(seg.parameters(), lr=0.006, weight_decay=0.05, fused=True)
    data = make_batch(rank, args.scenes, args.points, device, cfg["in_channels"], cfg["num_classes"])
    n_points = int(data["coord"].shape[0])
    autocast = torch.autocast("cuda", dtype=torch.bfloat16) if args.dtype == "bf16" else None
    basket = None
    if args.segmentor == "sam_image":
        # REAL's extra batch keys: scene names and the original index of every point; the basket holds whole scenes
        bounds = [0] + data["offset"].tolist()
        data["scene_id"] = ["Area_%d/room_%d.pth" % (rank + 1, i) for i in range(args.scenes)]
        data["instance"] = torch.cat([torch.randperm(2 * (b - a), device=device)[: b - a] for a, b in zip(bounds, bounds[1:])])
        data["offset_host"] = bounds[1:]
        basket = ptv2.LogitBasket({seg.scene_key(s): 2 * (b - a) for s, a, b in zip(data["scene_id"], bounds, bounds[1:])},
                                  cfg["num_classes"], device=device, max_rows=n_points)

    # geometry of batch i+1 (coordinates only) is built on a side stream during the backward of batch i, as a
    # loader would; every step still builds exactly one geometry (AO_AMD_PREFETCH=0: build it inline instead)
    # AO_AMD_PREFETCH=thread (default): built by a host thread of its own, started as soon as the current batch's geometry has
    # been handed over -- what a loader worker does.  It takes 2.75 ms of the 7.5 ms per step off the launching thread, which
    # otherwise runs only ~3.5 ms ahead of the GPU queue: on a quiet host both ways measure the same (10.93-11.06 ms, 24 paired
    # runs), on a slow one the launching thread is what the step waits for ("Host side").
    # =1: on the launching thread behind the backward (rounds 1-2); =0: in line
    prefetch, pf_mode = None, os.environ.get("AO_AMD_PREFETCH", "thread")
    if pf_mode in ("1", "thread"):
        prefetch = parallel.GeometryPrefetcher(seg.backbone, device, threaded=pf_mode == "thread")
        # thread mode: two geometries requested ahead -- the launching thread then finds the next one built instead of waiting for
        # the worker's read-backs, and a stall of either thread is absorbed by the other's lead.  Every step still builds one.
        for _ in range(2 if pf_mode == "thread" else 1):
            prefetch.start(data["coord"], data["offset"])

    ar_events = [] if sync is not None else None  # (event pair, bytes) per step around the gradient all-reduce

    def step():
        batch = data if prefetch is None else dict(data, geometry=prefetch.take())
        if prefetch is not None and pf_mode == "thread":
            prefetch.start(data["coord"], data["offset"])
        if autocast is not None:
            with autocast:
                out = net(batch)
        else:
            out = net(batch)
        if basket is not None:  # engines/train_sam_real.py:229-234, without its two blocking copies per scene
            out, seg_dict = out
            basket.put(seg_dict)
        loss = out["loss"]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if flat_opt:  # gradients -> one flat buffer -> (all-reduce) -> one update kernel
            flat = opt.flatten_grads()
            if sync is not None and ar_events is not None:  # the exchange bracketed on the stream that waits for it
                ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ea.record()
                scale = sync.reduce_flat(flat)
                eb.record()
                ar_events.append((ea, eb, flat.numel() * 4))
            else:
                scale = sync.reduce_flat(flat) if sync is not None else 1.0
            if prefetch is not None and pf_mode == "1":
                prefetch.start(data["coord"], data["offset"])
            opt.step(flat_grad=flat, grad_scale=scale)
            return loss
        if sync is not None:
            sync.sync()
        if prefetch is not None and pf_mode == "1":
            prefetch.start(data["coord"], data["offset"])
        opt.step()
        return loss

    # roofline leg: the last warm-up steps run with every hand-written kernel bracketed by HIP events to find the
    # dominant one; inside the timed region only every `timed_stride`-th launch of that kernel is bracketed (so the
    # step time the headline value comes from is not inflated by ~4000 event records)
    # The warm-up: first the survey steps (eager issue: HIP events cannot be read back from a graph), then the remaining
    # steps as the timed region will run them (graph issue, the dominant kernel sampled) so that the executable graphs exist
    if prefetch is not None and args.warmup > 0 and os.environ.get("AO_AMD_BENCH_POOL_WARM", "1") != "0":
        # The timed region lets the host run up to eight steps ahead of the GPU (the graph ring), the warm-up at most `warmup`
        # steps: the geometries of the steps in flight are memory the caching allocator cannot hand out again yet, and the first
        # time the host gets that far ahead it has to ask the driver for more (hipMalloc: a 70-130 ms stall of the launching
        # thread, seen as ONE long step in three of ~60 runs).  Untimed: hold eight geometries at once on the prefetch stream,
        # then let them go -- the allocator's pool of that stream is then as large as the run-ahead can make it.  (Twelve: the
        # eight steps of the graph ring, the two geometries the prefetcher keeps ahead, the one in use and one being freed; with
        # eight held the pool still grew by 74 MB in steps 8-11 of every timed region.)
        held = []
        for _ in range(12):
            prefetch.start(data["coord"], data["offset"])
        for _ in range(12):
            held.append(prefetch.take())
        torch.cuda.synchronize(device)
        del held
    survey_steps = 0 if args.no_roofline else min(2, args.warmup)
    survey, dominant, timed_stride = {}, None, 3
    # (no cyclic-garbage collection inside the timed region: a full collection of the interpreter's objects is tens of
    # milliseconds on the launching thread, which no training loop would let happen in the middle of a step either.  The
    # collection itself runs BEFORE the last warm-up steps, not between them and the timed region: tens of milliseconds of an
    # idle GPU there sent the first timed step off at idle clocks -- it took 1.25-1.3 x the median step at every size, 0.13-0.33
    # ms on the mean of 20.)
    import gc

    def gc_off():
        if gc.isenabled():
            gc.collect()
            gc.disable()

    if survey_steps:
        pre = 1 if args.warmup > survey_steps else 0
        for _ in range(pre):  # (one step before the survey when the warm-up allows: first-launch costs are not the kernels')
            step()
        torch.cuda.synchronize(device)
        _lib.kernel_timer(True)
        for _ in range(survey_steps):
            step()
        torch.cuda.synchronize(device)
        _lib.kernel_timer(False)
        survey = _lib.kernel_timer_read()
        if survey:
            # the dominant KERNEL: the largest total among the timer ids that bracket ONE kernel symbol (an instantiation, as
            # rocprofv3's per-kernel table lists it).  Ids whose name ends in " [family]" bracket several symbols -- the row GEMMs
            # of one column-block width, the kernels of a BatchNorm pass -- and are ranked as families in `all_kernels` only.
            single = {k: v for k, v in survey.items() if not k.endswith("[family]")}
            dominant = max((single or survey).items(), key=lambda kv: kv[1]["total_us"])[0]
            # every stride-th launch of it: a uniform sample over the timed region.  ~6 bracketed launches per step (a bracket
            # costs ~3 us of queue time: bracketing all 52 weight-gradient launches of a step was 0.1 ms of it); the stride is
            # co-prime with the launches per step so that the sampled positions spread over all Blocks
            import math
            per_step = max(1, round(survey[dominant]["launches"] / survey_steps))
            timed_stride = 3
            if per_step > 18:
                timed_stride = max(3, per_step // 6) | 1
                while math.gcd(timed_stride, per_step) != 1:
                    timed_stride += 2
            _lib.kernel_timer(True, only=dominant, stride=timed_stride)
        gc_off()
        for _ in range(args.warmup - survey_steps - pre):
            step()
        if survey:  # the records of the warm-up are not the timed region's
            _lib.kernel_timer(True, only=dominant, stride=timed_stride)
    else:
        gc_off()
        for _ in range(args.warmup):
            step()
    # host side of the timed region: wall and CPU time the launching thread spends inside step(), and one
    # event per step on the compute stream so that the per-step GPU-side durations can be told apart from host stalls
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    host_wall, host_cpu, reserved_trace = [], [], []
    captured = {}  # --dump-outputs: the backbone's output of the last timed step, copied (a runtime buffer may be reused)

    def timed_step():
        i = len(host_wall)
        if i == 0:
            marks[0].record()
        hook = None
        if args.dump_outputs and i == args.steps - 1:
            hook = seg.backbone.register_forward_hook(lambda m, a, y: captured.update(logits=y.detach().float().clone()))
        w0, c0 = time.perf_counter(), time.thread_time()
        out = step()
        if hook is not None:
            hook.remove()
        host_wall.append(time.perf_counter() - w0)
        host_cpu.append(time.thread_time() - c0)
        reserved_trace.append(torch.cuda.memory_reserved(device))
        marks[i + 1].record()
        return out

    if ar_events is not None:
        del ar_events[:]  # (the warm-up's)
    _lib.graph_stats(reset=True)
    cg0 = cgroup_cpu()[1]
    threads0, proc_cpu0 = thread_cpu_snapshot(), time.process_time()
    gc_off()
    reserved0 = torch.cuda.memory_reserved(device)
    try:
        elapsed, points_per_step, loss = parallel.timed_steps(timed_step, args.steps, device, n_points,
                                                              finish=basket.flush if basket is not None else None)
    finally:
        gc.enable()
    reserved_growth = torch.cuda.memory_reserved(device) - reserved0  # > 0: the caching allocator went to the driver while timed
    graph = _lib.graph_stats()
    cg1 = cgroup_cpu()[1]
    # what THIS rank's process cost the host inside the timed region (all ranks of a node share one cgroup CPU quota)
    threads1 = thread_cpu_snapshot()
    mine = {"rank": rank, "host_cpu_ms": 1e3 * sum(host_cpu) / max(len(host_cpu), 1),
            "host_issue_ms": 1e3 * sum(host_wall) / max(len(host_wall), 1),
            "process_cpu_ms_per_step": 1e3 * (time.process_time() - proc_cpu0) / args.steps, "threads": len(threads1),
            "busy_threads_ms_per_step": sorted(
                ([n, round(1e3 * (c - threads0.get(t, (n, 0.0))[1]) / args.steps, 3)] for t, (n, c) in threads1.items()
                 if c - threads0.get(t, (n, 0.0))[1] > 0.0), key=lambda kv: -kv[1])[:6]}
    per_rank = [mine]
    if dist.is_initialized() and world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    if prefetch is not None:
        prefetch.close()  # (thread mode: the geometry of the batch after the last one is still being built)
    if args.dump_outputs and rank == 0:
        params = list(seg.parameters())
        written = dump_outputs(args.dump_outputs, {
            "loss": loss.detach().reshape(1), "logits": captured["logits"],
            "params": torch.cat([p.detach().reshape(-1) for p in params]),
            "grads": torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params]),
            "buffers": torch.cat([b.detach().float().reshape(-1) for b in seg.buffers()])})
        sys.stderr.write("bench.py: outputs of the last timed step in %s: %s\n" % (args.dump_outputs, json.dumps(written)))
    if not args.no_roofline:
        _lib.lib().ptv2_profile_enable(0)
    ref_loop = None
    if not args.no_reference_loop:  # every rank takes part (DistributedDataParallel at world_size > 1)
        try:
            ref_loop = reference_loop_leg(ptv2, args, cfg, device, data, world, points_per_step)
        except Exception as exc:  # (after the timed region: a failure here is reported on the line, it does not take the headline down)
            if world > 1:
                raise  # (the other ranks are inside its collectives: fail together, loudly)
            ref_loop = {"error": repr(exc)[:300]}

    if rank == 0:
        with torch.no_grad():
            geo = seg.backbone.geometry(data["coord"], data["offset"])
        levels = [int(lv.coord.shape[0]) for lv in geo.levels]
        ms = 1e3 * elapsed / args.steps
        build_info = _lib.lib().ptv2_build_info().decode()
        out = {
            "metric": "points/sec fwd+bwd PTv2m2 S3DIS" if args.cfg == "s3dis" else "points/sec fwd+bwd PTv2m2 ScanNet cfg", "value": points_per_step * args.steps / elapsed,
            "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            # the arithmetic type of the matrix products: fp32 MFMA (headline), or under --dtype bf16 (torch.autocast, the
            # reference trainer's enable_amp) bf16 MFMA operands with fp32 accumulation; storage is fp32 in both
            "dtype": "bf16" if (args.dtype == "bf16" and os.environ.get("AO_AMD_AUTOCAST_MATMUL", "bf16") == "bf16") else "fp32",
            "data": "synthetic",
            "config": {"workload": "%s semseg-pt-v2m2-0-base, %d scene(s)/GPU x %d pts, train step "
                                   "(geometry+fwd+CE+bwd+AdamW), drop_path 0.3" % (args.cfg, args.scenes, args.points),
                       "points_per_gpu": n_points, "level_sizes": levels, "gva": os.environ.get("AO_AMD_GVA", "default"),
                       "autocast": args.dtype if args.dtype != "fp32" else None,
                       "precision": ("Linear products on bf16 MFMA (operands rounded to bf16, fp32 accumulate); activations, "
                                     "BatchNorm statistics, softmax, coordinates fp32" if args.dtype == "bf16" else
                                     "fp32 MFMA (exact fp32) everywhere"), "parallelism": "dp%d" % world,
                       "rccl_ranks": dist.get_world_size() if dist.is_initialized() else 1,
                       "comm_backend": (dist.get_backend() if dist.is_initialized() else None),
                       "launcher": _launcher_name(),
                       "miou": "not measured: no S3DIS on the box.  The 'mIoU within +-0.2 after equal steps' target of BASELINE.json has "
                               "a synthetic stand-in only (tests/test_gpu_model.py: 10-step trajectory vs the CPU oracle, 150 steps vs "
                               "the literal op sequence)",
                       "grad_sync": "ddp" if use_ddp else ("flat all-reduce, two chunks (decoder half overlapped with the encoder "
                                                             "backward)" if (sync is not None and sync.split is not None)
                                                            else "flat all-reduce"),
                       "optimizer": "FlatAdamW (one kernel)" if flat_opt else "torch.optim.AdamW(fused)",
                       # what this line's loop uses that the reference trainer's own loop does not (INTEGRATION.md section 3b':
                       # optional accelerations; `reference_loop` below is the number without any of them)
                       "trainer_side": ([] if prefetch is None else ["GeometryPrefetcher (%s): the next batch's geometry on a side stream, "
                                                                      "handed over as batch['geometry']" % pf_mode])
                                       + (["FlatAdamW", "native_param_grads=%s" % seg.backbone.native_param_grads] if flat_opt else [])
                                       + (["FlatGradSync (one flat all-reduce)"] if sync is not None else []),
                       "segmentor": "DefaultSegmentorSAM_Image + LogitBasket (%d puts, %d waits for a staging slot)"
                                    % (basket.puts, basket.waits) if basket is not None else "DefaultSegmentor",
                       "loss": float(loss.detach()), "library_build": "src " + str(src_hash(build_info))},
        }
        first_step_ms = marks[0].elapsed_time(marks[1])
        step_ms_in_order = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        step_ms = sorted(step_ms_in_order)
        pick = lambda q: step_ms[min(len(step_ms) - 1, int(q * len(step_ms)))]
        out["host"] = host_facts()
        out["host"].update({
            # time the launching thread spends inside one step (wall: includes waiting for a full queue / the geometry
            # thread; cpu: time.thread_time of that thread) against the step time -- host-bound when they approach it
            "host_issue_ms": 1e3 * sum(host_wall) / len(host_wall), "host_issue_ms_max": 1e3 * max(host_wall),
            "host_cpu_ms": 1e3 * sum(host_cpu) / len(host_cpu),
            # per-step durations between events recorded on the compute stream at the end of every step
            # (`first`: the step behind the synchronisation that opens the timed region -- the GPU idles while the host captures,
            # updates and launches the forward's graph, and runs the step's first milliseconds from a cold start)
            "step_ms": {"min": step_ms[0], "median": pick(0.5), "p90": pick(0.9), "max": step_ms[-1], "first": first_step_ms,
                        "in_order": [round(x, 2) for x in step_ms_in_order[:64]]},
            "issue": ("hipGraph: each direction of the model captured and launched as one graph (ao_amd/csrc/graph.hip)"
                      if graph["scopes"] > 0 else "eager (hipLaunchKernelGGL per kernel)"),
            "graph": {"launches_per_step": graph["scopes"] / args.steps, "nodes_per_step": graph["nodes"] / args.steps,
                      "updated_in_place": int(graph["updated"]), "instantiated": int(graph["instantiated"]),
                      "ran_eagerly": int(graph["declined"]),
                      "capture_ms_per_step": 1e-3 * graph["capture_us"] / args.steps,
                      "update_ms_per_step": 1e-3 * graph["update_us"] / args.steps,
                      "launch_ms_per_step": 1e-3 * graph["launch_us"] / args.steps,
                      "wait_for_gpu_ms_per_step": 1e-3 * graph["wait_us"] / args.steps},
            "geometry_prefetch": pf_mode,
            # every rank's host cost inside the timed region: CPU of its launching thread, of its whole process (geometry
            # worker, HIP / RCCL helper threads included), its busiest threads -- N ranks share the node's cgroup quota
            "per_rank": per_rank,
            # the cgroup's CPU accounting across the timed region: a throttled period there is a stalled launching thread
            "cgroup_timed_region": ({k: cg1[k] - cg0[k] for k in cg1 if k in cg0} if cg0 and cg1 else None),
            # bytes torch's caching allocator obtained from the driver inside the timed region (hipMalloc blocks the launching thread)
            "allocator_reserved_growth_MB": round(reserved_growth / 2 ** 20, 1),
            "allocator_reserved_MB_after_step": [round(r / 2 ** 20) for r in reserved_trace[:12]],
            "allocator_reserved_MB_before": round(reserved0 / 2 ** 20),
            "torch_cpu_threads": torch.get_num_threads()})
        step_bytes = algorithmic_step_bytes(levels, cfg)
        out["config"]["algorithmic_step_GB"] = step_bytes / 1e9
        out["config"]["step_frac_of_hbm_roofline"] = (step_bytes / (ms * 1e-3)) / (HBM_PEAK_GBS * 1e9)
        if not args.no_roofline:
            summ = _lib.kernel_timer_read()
            if summ and dominant in summ:
                # dominant hand-written kernel of the step (largest total time in the survey steps), timed live
                # over the timed region
                name, rec = dominant, summ[dominant]
                # a bracket is [event record, kernel, event record] on the launch stream: its elapsed time contains the two
                # records' own queue time.  Calibrated here as the median elapsed time of 200 EMPTY brackets on the same stream
                # and subtracted, so that the figure is comparable with rocprofv3's kernel duration (profiles/*_kernel_summary)
                pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(200)]
                for a, b in pairs:
                    a.record()
                    b.record()
                torch.cuda.synchronize(device)
                empty_us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)[len(pairs) // 2]
                bracket = "HIP events"
                if graph["scopes"] > 0:
                    # graph issue: the brackets of the timed region were pairs of device time-stamp kernels inside the captured
                    # sequence (an event-record node cannot be read back); calibrate with empty stamp brackets in a graph
                    bracket = "device time stamps (wall_clock64) inside the graph; the survey steps used HIP events, eager issue"
                    e2 = _lib.lib().ptv2_profile_empty_stamp_us(torch.cuda.current_stream(device).cuda_stream, 200)
                    if e2 >= 0:
                        empty_us = e2
                net_us = max(rec["avg_us"] - empty_us, 0.5 * rec["avg_us"])
                achieved = rec["bytes_per_launch"] / (net_us * 1e-6) / 1e9
                traffic, traffic_source = pmc_traffic(name, build_info)
                flops = mfma_bound_flops(name, levels)
                head = ({"bound": "mfma", "kernel": name, "achieved": flops / (net_us * 1e-6) / 1e12, "peak": MFMA_FP32_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": flops / (net_us * 1e-6) / 1e12 / MFMA_FP32_PEAK_TFLOPS,
                         "algorithmic_flops_per_launch": flops, "hbm_achieved_GBps": achieved, "hbm_frac": achieved / HBM_PEAK_GBS,
                         "why_mfma": "the deep-level attention tile kernels keep their operands in LDS / registers (a few MB from "
                                     "memory per launch): the exact-fp32 matrix pipe bounds them"}
                        if flops else
                        {"bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS})
                out["roofline"] = {**head, "traffic": traffic,
                                   "traffic_source": traffic_source,
                                   "avg_us": net_us, "avg_us_bracket": rec["avg_us"], "empty_bracket_us": empty_us,
                                   "bracket": bracket,
                                   "avg_us_survey_hip_events": (round(survey[name]["avg_us"], 2) if name in survey else None),
                                   "launches_timed": rec["launches"],
                                   "ms_per_step": timed_stride * rec["total_us"] / 1e3 / args.steps,
                                   "algorithmic_bytes_per_launch": rec["bytes_per_launch"],
                                   "survey_steps": survey_steps, "timed_launch_stride": timed_stride,
                                   # the next families by time, from the survey steps (HIP events, eager issue), same definitions
                                   "next": [dict(kernel=k, achieved=round(v["bytes_per_launch"] / (v["avg_us"] * 1e-6) / 1e9, 1),
                                                 frac=round(v["bytes_per_launch"] / (v["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 3),
                                                 avg_us=round(v["avg_us"], 1), launches_per_step=v["launches"] / max(survey_steps, 1),
                                                 traffic=pmc_traffic(k, build_info)[0])
                                            for k, v in [kv for kv in sorted(survey.items(), key=lambda kv: -kv[1]["total_us"])
                                                         if kv[0] != dominant][:3]],
                                   "all_kernels": {k: {"avg_us": round(v["avg_us"], 2), "launches": v["launches"],
                                                       "ms_per_step": round(v["total_us"] / 1e3 / max(survey_steps, 1), 3),
                                                       "GBps": round(v["bytes_per_launch"] / (v["avg_us"] * 1e-6) / 1e9, 1)}
                                                   for k, v in sorted(survey.items(), key=lambda kv: -kv[1]["total_us"])}}
        if ar_events:
            # per-step gradient exchange from events on the stream that waits for it: what the first real N > 1 line needs to
            # explain itself.  Bus bandwidth as nccl-tests define it for an all-reduce: 2 (N - 1) / N x bytes / time
            ms_list = sorted(a.elapsed_time(b) for a, b, _ in ar_events)
            nbytes = ar_events[0][2]
            med = ms_list[len(ms_list) // 2]
            out["config"]["all_reduce"] = {"ms_per_step_median": med, "ms_per_step_max": ms_list[-1], "MB": nbytes / 1e6,
                                           "bus_GBps": (2.0 * (world - 1) / world) * nbytes / (med * 1e-3) / 1e9 if world > 1 and med > 0 else None,
                                           "ranks": world, "what": "HIP events around FlatGradSync.reduce_flat on rank 0's compute stream "
                                           "(the collective runs on RCCL's stream; the compute stream waits for it)"}
        if world == 1 and not args.no_roofline and args.cfg == "s3dis":
            try:
                out["roofline"]["block"] = block_leg(ptv2, geo, device)
                out["roofline"]["block_frac"] = out["roofline"]["block"]["backward"]["frac"]
            except Exception as exc:
                out.setdefault("roofline", {})["block"] = {"error": repr(exc)[:200]}
        if ref_loop is not None:
            out["reference_loop"] = ref_loop
        if world == 1 and not args.no_also and args.cfg == "s3dis" and args.scenes == 1 and args.points == 120000:
            out["config"]["also"] = also_leg(args)
        if world == 1 and not args.no_ops:
            out["ops"] = op_microbench(data)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg, args.cpu_sample_points)
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
