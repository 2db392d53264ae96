#!/usr/bin/env python3
"""Headline benchmark: warped+composited frames/sec at 256x512, 8 layers, fwd+bwd.

    python bench.py --gpus 1 --steps 100 --warmup 10           # config C3, the headline
    python bench.py --gpus 1 --steps 100 --warmup 10 --full    # ... with roofline, variants and CPU baseline
    python bench.py --steps 20 --warmup 5 --dump-outputs DIR   # ... and the last step's outputs as DIR/*.npy
    python bench.py --config C5                                # the other BASELINE.json configs
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[2], SURVEY.md 8(d) "C3"): per rank B clips x T=14 frames,
L=8 layers of 4x256x512 (RGB+alpha in [-1,1]), 16 TPS control points per layer,
occ = compute_occ(randn).  One step = one pass of the hot path over that batch:
  fwd  rgb = warp_composite(layers, pts, occ)      (TPS grid -> bilinear warp -> reduce_comp)
  bwd  rgb.square().mean().backward()              grads on layers and control points (the loss as written: autograd's
                                                   own gradient chain is inside the timed step)
Inputs are resident in HBM when the timed region starts.  Frames are independent, so ranks shard
them with no data-path collective ("scaling": "weak", per-GPU work fixed).

Named workloads (--config; BASELINE.json `configs`); C3 is the default and the
only one the headline metric is quoted on, the others print the same JSON shape with their own
metric string:
  C2  8 frames of 128x128, L=8, forward only (launch-bound: replayed from a HIP graph)
  C3  8 clips x 14 frames of 256x512, L=8, fwd+bwd
  C4  8 clips x 9 frames of 256x832 (KITTI), L=8, forward + all-gather of the composited frames
  C5  4 clips x 14 frames of 512x1024, L=12, forward + all-gather
  LVD 2 clips x 5 frames of 128x256, L=17: the warp-path part of an LVD training step (the reference's live
      backward path, models/synthesizer.py:815-841), fwd+bwd, per-entry-point table
  WIF 2 clips x 5 frames (4 context + 1 predicted) of 512x1024 over 128x256 layers, L=17: BASELINE config 3 as the
      reference RUNS it (Synthesizer.inpaint, models/synthesizer.py:517-576, 631-633): the unrestricted grid_to_flow +
      input_to_output under no_grad, then WIF.forward + backward; per-entry-point table
  (--pipeline with C4 / C5: Synthesizer.predict's hot-path calls on whole clips instead of the synthetic forward)

Timing protocol of every workload: a time-based settle (>= 0.3 s of the step, `settle_ms`) before the --warmup steps,
then ONE block of exactly --steps steps, bracketed by barrier + synchronize; `ms_per_step` is that block's time per
step (max over ranks).  A plain run does nothing else: it sets up, warms up, times the --steps steps, writes the outputs
(--dump-outputs) and prints the headline line.

--full adds everything beyond the headline, as before: FIVE blocks of exactly --steps steps, `ms_per_step` the MEDIAN
block (`ms_per_step_blocks` lists all five, max over ranks each), and the figures that take passes of their own -- the
per-kernel event pairs (taken in a separate pass afterwards, so the timed blocks carry no events), the roofline, the
HIP-graph / loss-gradient / decode variants beside the headline, the CPU baseline and, with --gpus N > 1 and the
default workload, a `north_star` object (the RCCL all-gather of composited frames, the C5 pipeline as ONE job split over
the N ranks, a cross-rank bit-equality check): see north_star_block.

--dump-outputs DIR writes what the timed path handed its caller in the LAST timed step (the composited frames, the
loss and the gradients of a training step) as DIR/<name>.npy in float32, at most 64 MB in all (dump_outputs: a fixed,
seeded sample of a larger array).  The inputs are seeded: the same arguments give the same inputs on every run.

Prints ONE JSON line on rank 0 (contract in the task statement); with --full it carries two extra objects:
  roofline      dominant kernel, algorithmic bytes per launch / mean launch duration measured live
                with events on the launch stream, against the 8 TB/s HBM3E peak
  cpu_baseline  the oracle (a PyTorch-CPU restatement of the reference path, oracle/wif_oracle.py)
                timed on this host's cores on a bounded sample of the same workload
"""
import argparse
import gc
import json
import os
import sys
import time

if len(sys.argv) > 7 and sys.argv[1] == "--cpu-baseline-child" and hasattr(os, "sched_setaffinity"):
    # the CPU-baseline child pins itself BEFORE torch is imported (its thread pools size themselves from the mask)
    _allowed = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, set(_allowed[:max(1, min(int(sys.argv[7]), len(_allowed)))]))

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def synth(frames, nl, h, w, device, seed, sigma=0.05):
    """Same recipe as oracle.wif_oracle.make_synthetic, generated on the device."""
    from waldo_amd.tools.utils import get_grid
    g = torch.Generator(device=device).manual_seed(seed)
    layers = torch.rand(frames, nl, 4, h, w, generator=g, device=device) * 2 - 1
    ctrl = get_grid(4, 4).view(1, 16, 2).to(device)
    pts = ctrl + sigma * torch.randn(frames * nl, 16, 2, generator=g, device=device)
    score = torch.randn(frames, nl - 1, generator=g, device=device)
    s = torch.exp(-score ** 2) + 1e-6
    occ = torch.zeros(frames, nl, nl, device=device)
    occ[:, 1:, 1:] = s[:, :, None] / (s[:, :, None] + s[:, None, :]) - 0.5 * torch.eye(nl - 1, device=device)
    occ[:, 1:, 0] = 1.0
    return layers, pts, occ


class _SquareMean(torch.autograd.Function):
    """The benchmark's loss, out.square().mean(), with its gradient 2 * out / N written as
    ONE elementwise kernel: autograd's own chain for it (expand, copy, two multiplies) is four passes
    over the 176 MB output, ~0.2 ms per step of pure loss scaffolding at the headline shape."""

    @staticmethod
    def forward(ctx, out):
        ctx.save_for_backward(out)
        return out.square().mean()

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return out * (g * (2.0 / out.numel()))


def copy_bandwidth(device, nbytes=1 << 30, reps=10):
    """Measured device-to-device copy rate of this box (read + write bytes per second, GB/s): the
    second denominator SURVEY 8(d) asks for next to the 8 TB/s spec figure."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def cpu_budget():
    """CPUs this process may really use: its affinity mask, cut to the cgroup's CPU quota when there is one (a
    box that shows 256 logical CPUs but grants 16 CPUs' worth of time throttles a 32-thread run -- the 3.7x spread
    of round 3's baseline)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as fh:
                txt = fh.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                        n = min(n, max(1, q // int(fh.read())))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline_child(argv):
    """``bench.py --cpu-baseline-child NL H W FRAMES REPS THREADS``: one measurement of the oracle in a process of
    its own, pinned BEFORE torch starts (affinity mask of THREADS CPUs, OMP_PROC_BIND / OMP_PLACES from the parent's
    environment), printing one JSON object: seconds of every repetition after a warm-up.  Never touches the GPU."""
    nl, h, w, frames, reps, threads = (int(x) for x in argv)
    torch.set_num_threads(threads)  # (the affinity mask was set at the top of this file, before `import torch`)
    from oracle import wif_oracle as O
    layers, pts, occ, inv, rep = O.make_synthetic(frames, nl, h, w, seed=0)
    lay, pt = layers.clone().requires_grad_(), pts.clone().requires_grad_()

    def once():
        lay.grad = pt.grad = None
        t0 = time.perf_counter()
        rgb, _ = O.warp_composite(lay, pt, occ, inv, rep)
        rgb.square().mean().backward()
        return time.perf_counter() - t0

    once()
    print(json.dumps({"seconds": [once() for _ in range(reps)]}), flush=True)


def cpu_throttle_counters():
    """cgroup CPU statistics of this container (cpu.stat: nr_periods, nr_throttled, throttled_usec / throttled_time),
    or {}: what tells a quota-throttled measurement from one disturbed by other tenants of the host."""
    for path in ("/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat", "/sys/fs/cgroup/cpu,cpuacct/cpu.stat"):
        try:
            with open(path) as fh:
                out = {}
                for ln in fh:
                    k, _, v = ln.partition(" ")
                    if k in ("nr_periods", "nr_throttled", "throttled_usec", "throttled_time", "usage_usec"):
                        out[k] = int(v)
                return out
        except (OSError, ValueError):
            continue
    return {}


def cpu_baseline(nl, h, w, frames, reps):
    """Oracle (kind "port") on the host cores: fwd+bwd frames/s on `frames` frames.

    Every measurement runs in a CHILD process that is pinned before torch starts (OMP_NUM_THREADS, OMP_PROC_BIND=close,
    OMP_PLACES=cores, an affinity mask of as many CPUs as threads), with thread counts that fit the CPU time the box
    really grants (`cpu_budget`: affinity cut to the cgroup quota).  The thread count is the best median of three
    on the same sample among a FIXED list; the figure is the median of the LAST `reps` runs at that count, and batches of
    `reps` runs are repeated (at most three) until worst / best of a batch is <= 1.3.  The cgroup's throttling counters
    are read before and after and printed: `unstable: true` (worst / best still > 1.3, or the probe and the measurement
    at that thread count disagree by more than 1.5x) comes with the counter that explains it, or says that none moved."""
    import subprocess
    budget = cpu_budget()

    def child(nf, n_rep, threads):
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), OMP_PROC_BIND="close",
                   OMP_PLACES="cores", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", str(nl), str(h), str(w),
                            str(nf), str(n_rep), str(threads)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"cpu baseline child failed: {r.stderr[-1000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["seconds"]

    def median(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    before = cpu_throttle_counters()
    cands = [c for c in (4, 8, 16, 32) if c <= budget] or [budget]
    probe = {c: median(child(frames, 3, c)) for c in cands}  # the SAME sample as the measurement
    cores = min(probe, key=probe.get)
    batches = []
    for _ in range(3):
        batches.append(sorted(child(frames, max(reps, 3), cores)))
        if batches[-1][-1] / batches[-1][0] <= 1.3:
            break
    times = batches[-1]
    med = median(times)
    f1 = max(1, min(4, frames))
    t1 = median(child(f1, 3, 1))
    after = cpu_throttle_counters()
    delta = {k: after[k] - before[k] for k in after if k in before}
    spread = times[-1] / times[0]
    disagree = max(med, probe[cores]) / min(med, probe[cores])  # two runs of one configuration, minutes apart
    unstable = bool(spread > 1.3 or disagree > 1.5)
    if delta.get("nr_throttled", 0) > 0:
        why = (f"cgroup CPU quota: throttled in {delta['nr_throttled']} of {delta.get('nr_periods', '?')} periods during the "
               f"baseline ({delta.get('throttled_usec', delta.get('throttled_time', 0))} "
               f"{'us' if 'throttled_usec' in delta else 'ns'} throttled)")
    elif delta:
        why = ("no cgroup throttling during the baseline (nr_throttled unchanged): the spread comes from outside this "
               "container -- other tenants of the shared host (steal time is not visible from inside)")
    else:
        why = "cpu.stat not readable in this container: cause of the spread unknown"
    out = {"value": round(frames / med, 3), "unit": "frames/s", "cores": cores, "kind": "port",
           "value_best": round(frames / times[0], 3), "value_worst": round(frames / times[-1], 3),
           "worst_over_best": round(spread, 3), "batches_run": len(batches),
           "unstable": unstable, "spread_explained_by": why if unstable else None,
           "cpu_stat_delta": delta or None,
           "probe_over_measurement": round(probe[cores] / med, 3),
           "value_1_thread": round(f1 / t1, 3), "cpu_budget": budget,
           "thread_probe_frames_per_s": {str(c): round(frames / t, 3) for c, t in probe.items()},
           "sample": f"{frames} frames of the same workload ({nl}x4x{h}x{w}, fwd+bwd), "
                     f"median of the last batch of {len(times)} runs after warm-up (best / worst beside it; batches are "
                     f"repeated, at most 3, until worst / best <= 1.3), torch {torch.__version__} "
                     f"CPU in a pinned child process (OMP_PROC_BIND=close, affinity = {cores} CPUs), {cores} threads = "
                     f"best median of 3 on the same {frames} frames among {cands} (CPU budget {budget} of "
                     f"{os.cpu_count()} logical CPUs); unstable = worst / best > 1.3 or the probe and the measurement at "
                     f"{cores} threads disagree by more than 1.5x; value_1_thread: {f1} frames, median of 3"}
    return out


# kernels behind the two entry points of the fused path, as rocprofv3 names them
_TRAFFIC_KERNELS = {"waldo_warp_composite_fwd": ("warp_composite_fwd_lds_kernel", "warp_composite_fwd_kernel"),
                    "waldo_warp_composite_bwd": ("warp_composite_bwd_px16_kernel", "warp_composite_splat_kernel",
                                                 "warp_composite_gmap_reduce_kernel", "warp_composite_bwd_kernel")}


def live_traffic(argv, timeout=240):
    """HBM-side bytes per launch of the fused path's entry points, measured NOW: this command again (three steps, no
    baselines) as a child under ``rocprofv3 --kernel-trace --pmc FETCH_SIZE`` and, in a second pass, ``--pmc WRITE_SIZE``
    (the two do not fit one pass; MI355X_MICROARCH.md: the counters sit on the L2's fabric side, are reported in KiB, and
    on gfx950 FETCH_SIZE tallies a 128-byte request of a wide coalesced read as 64 bytes -- doubled here -- while
    WRITE_SIZE is exact for 16-byte streaming stores).  Returns {entry point: bytes per launch} or raises."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        raise RuntimeError("rocprofv3 not found")
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        raise RuntimeError("this run is itself under a profiler")
    per = {k: 0.0 for k in _TRAFFIC_KERNELS}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        for counter, factor in (("FETCH_SIZE", 2.0 * 1024.0), ("WRITE_SIZE", 1024.0)):
            out = os.path.join(tmp, counter)
            cmd = [prof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.abspath(__file__)] + argv
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True,
                               timeout=timeout)
            rows = {}
            for f in glob.glob(os.path.join(out, "*", "*counter_collection.csv")):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if row["Counter_Name"] == counter:
                            rows.setdefault(row["Kernel_Name"].split("(")[0], []).append(float(row["Counter_Value"]))
            if not rows:
                raise RuntimeError(f"no {counter} rows (rocprofv3 rc {r.returncode}): {r.stderr[-300:]}")
            for entry, kernels in _TRAFFIC_KERNELS.items():
                for name, vals in rows.items():
                    if any(name.endswith("::" + k) or ("::" + k + "<") in name for k in kernels):
                        per[entry] += sum(vals) / len(vals) * factor
    return per


def measured_traffic(entry_point, frames, nl, h, w):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/traffic.json, written
    by tools_dev/traffic.py from FETCH_SIZE / WRITE_SIZE with the gfx950 corrections of
    MI355X_MICROARCH.md), if one matches this workload; else null."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(path) as fh:
            t = json.load(fh)
        if t.get("frames") == frames and t.get("layers") == nl and t.get("height") == h and t.get("width") == w:
            return t["bytes_per_launch"].get(entry_point)
    except (OSError, ValueError, KeyError):
        pass
    return None


CONFIGS = {
    # name: (clips per GPU, frames per clip, layers, height, width, mode)
    "C2": (1, 8, 8, 128, 128, "fwd"),
    "C3": (8, 14, 8, 256, 512, "train"),
    "C4": (8, 9, 8, 256, 832, "infer"),
    "C5": (4, 14, 12, 512, 1024, "infer"),
    # the reference's live backward path: the warp-path part of an LVD training step (waldo_amd/tools/lvd_step.py)
    "LVD": (2, 5, 17, 128, 256, "lvd"),
    # BASELINE config 3 as the reference runs it: Synthesizer.inpaint's call order at the train_wif.sh recipe
    # (waldo_amd/tools/wif_step.py): the warp path under no_grad, then WIF.forward + backward
    "WIF": (2, 5, 17, 512, 1024, "wif"),
}

TIMED_BLOCKS = 5       # --full: blocks of --steps steps; the median block is the line's ms_per_step
SETTLE_SECONDS = 0.3   # of the step itself, before the --warmup steps (a cold box: clocks, caches, allocator)
DUMP_BYTES = 64 * 10 ** 6  # --dump-outputs: every array of the dump together, .npy headers included


def timed_block_count(args):
    """A plain run times ONE block of exactly --steps steps; --full the median of TIMED_BLOCKS."""
    return TIMED_BLOCKS if args.full else 1


def dump_outputs(out_dir, arrays):
    """--dump-outputs: `arrays` (name -> tensor: what the timed path handed its caller in its last step) as
    out_dir/<name>.npy, float32 (float64 stays float64).  Each array gets an equal share of DUMP_BYTES; one larger than
    its share is written as a fixed sample -- its elements at flat indices drawn, sorted, from a CPU generator seeded
    with 0 -- so that the same arguments sample the same elements on every run and two builds compare element for
    element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = (DUMP_BYTES - 4096 * len(arrays)) // len(arrays)
    for name, t in arrays.items():
        t = t.detach()
        if t.dtype != torch.float64:
            t = t.float()
        cap = share // t.element_size()
        if t.numel() > cap:
            idx = torch.randint(t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
            arr = t.reshape(-1)[idx.to(t.device)].cpu().numpy()
        else:
            arr = t.cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def settle_interpreter():
    """Called after the warm-up, before a timed region: a full collection now, then everything that survives
    (the import-time heap of torch: ~10^6 container objects) is moved to the permanent generation, so that a
    generation-2 pass of Python's cyclic collector inside the timed region -- 50 ms on this stack, measured with
    tools_dev/lvd_dbg.py: 20 steps' worth -- has next to nothing to traverse.  The collector stays enabled."""
    gc.collect()
    gc.freeze()


def settle_gpu(step, fence, seconds=SETTLE_SECONDS):
    """Run the step for at least `seconds` (disclosed as `settle_ms`): the driver's `--warmup 5` is 16 ms of GPU work
    on a box that was idle a moment ago -- clocks, caches and the allocator have not seen the workload yet."""
    fence()
    t0 = time.perf_counter()
    while True:
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            break
    fence()
    return round((time.perf_counter() - t0) * 1e3, 1)


def timed_blocks(step, fence, steps, dist=None, device=None, backend="nccl", nblocks=TIMED_BLOCKS, between=None):
    """`nblocks` timed regions of EXACTLY `steps` steps, each bracketed by barrier + synchronize (`fence`); returns the
    blocks' seconds, the MAX over ranks of each.  No events are recorded inside them.  `between` (untimed) runs before
    every block."""
    blocks = []
    for _ in range(nblocks):
        if between is not None:
            between()
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        fence()
        blocks.append(time.perf_counter() - t0)
    if dist is not None:
        t = torch.tensor(blocks, device=device if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        blocks = t.tolist()
    return blocks


def median_block(blocks):
    return sorted(blocks)[len(blocks) // 2]


def block_fields(blocks, steps, settle_ms):
    if len(blocks) == 1:  # a plain run
        return {"settle_ms": settle_ms,
                "timing": f"one block of {steps} steps (bracketed by barrier + synchronize, max over ranks), after "
                          f"{settle_ms} ms of settling and the warm-up steps"}
    return {"ms_per_step_blocks": [round(b / steps * 1e3, 4) for b in blocks], "settle_ms": settle_ms,
            "timing": f"median of {len(blocks)} blocks of {steps} steps (each bracketed by barrier + synchronize, max over "
                      f"ranks), after {settle_ms} ms of settling and the warm-up steps; per-kernel events in a separate pass"}


def spawn_ranks(n):
    """One process per GPU, as the reference's launch scripts do (scripts/cityscapes/demo.sh:6-12: torchrun around
    the helper; tools/engine.py:28-35 reads the rank from the environment): the same command line under
    ``python -m torch.distributed.run`` on 127.0.0.1.  Returns the launcher's exit code."""
    import subprocess
    # the launcher picks the rendezvous port itself (c10d store on 127.0.0.1, port 0): no bind-close-reuse race when
    # several benches or tests start at once
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--rdzv-backend=c10d", "--rdzv-endpoint=127.0.0.1:0", "--local-addr=127.0.0.1",
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL / tensor sharing between the ranks
    return subprocess.run(cmd, env=env).returncode


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-child":
        cpu_baseline_child(sys.argv[2:8])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C3",
                    help="BASELINE.json workload; C3 (the default) is the one the headline metric is quoted on")
    ap.add_argument("--clips", type=int, default=None, help="clips per GPU (overrides the config)")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--frames-per-clip", type=int, default=None)
    ap.add_argument("--sigma", type=float, default=0.05, help="control-point noise (the benchmark is 0.05)")
    ap.add_argument("--mode", choices=["train", "infer", "fwd"], default=None,
                    help="train: fwd+bwd (the headline metric); infer: fwd only + RCCL all-gather of the "
                         "composited frames; fwd: forward only, replayed from a HIP graph")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL on ROCm) is the real thing; gloo only to smoke-test the "
                         "multi-rank code path on a box with fewer GPUs than ranks")
    ap.add_argument("--pipeline", action="store_true",
                    help="C4 / C5 only: the whole chain of Synthesizer.predict around the path (producers -> "
                         "Warper.forward -> decode_output -> WIF fusion) on whole clips, instead of the synthetic "
                         "fused forward (waldo_amd/tools/pipeline.py)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="--pipeline: weak = every rank keeps its own `clips` whole clips (per-GPU work fixed); strong = "
                         "the config's clips are ONE job whose (b, t) output frames are dealt over the ranks in "
                         "contiguous blocks (context frames replicated, one all-gather of the predicted frames), so that "
                         "a single clip uses every GPU (waldo_amd/tools/demo.py:predict_sharded)")
    ap.add_argument("--graph", action="store_true",
                    help="--pipeline / --config LVD: replay the rank's whole step from ONE HIP graph (the collective stays "
                         "outside it); the LVD step is ~90 short launches and its eager time follows the box's host")
    ap.add_argument("--shard", default=None, metavar="R/W",
                    help="--pipeline --scaling strong on ONE GPU: time rank R's share of a W-rank job without any "
                         "collective (what a rank of the 8-GPU node would compute; tools_dev/strong_projection.py)")
    ap.add_argument("--motion", choices=["calibrated", "wild"], default="calibrated",
                    help="--pipeline: background motion of the stand-in pose heads (waldo_amd/tools/demo.py:BG_MOTION); "
                         "'wild' is the folded warp rounds 1-3 benchmarked on, 'calibrated' keeps the local stretch of "
                         "the warp within what optical flow of the reference's demo clips shows")
    ap.add_argument("--debug-option", type=int, action="append", default=[],
                    help="set a test-only kernel-variant switch of the C ABI (include/waldo_hip.h: WALDO_DEBUG_*) for A/B "
                         "timing")
    ap.add_argument("--lib", default=None, help="A/B timing: another build of the library (tools_dev/build_variant.py)")
    ap.add_argument("--north-star", choices=["auto", "on", "off"], default="auto",
                    help="append the `north_star` object (all-gather of composited frames over the ranks, the C5 pipeline "
                         "as ONE job split over them, cross-rank bit-equality) to the default workload's line; auto: with "
                         "--full and --gpus > 1")
    ap.add_argument("--north-star-config", choices=["C4", "C5"], default="C5",
                    help="recipe of the north_star block's pipeline job (C5 = Cityscapes 512x1024, the north star's)")
    ap.add_argument("--fresh-inputs-per-block", action="store_true",
                    help="experiment: free and re-create the workload's tensors before every timed block (does the "
                         "placement of the buffers explain run-to-run differences of a few per cent?)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="roofline.traffic from the committed profiles/traffic.json instead of two rocprofv3 --pmc child "
                         "runs of this command (FETCH_SIZE, WRITE_SIZE: ~40 s)")
    ap.add_argument("--cpu-frames", type=int, default=28)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: five timed blocks (median), per-kernel table, roofline, the "
                         "variants beside the headline, CPU baseline, north_star (--gpus > 1); a plain run times one "
                         "block of --steps steps and prints the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path computed in its last timed step as DIR/<name>.npy (float32, at most "
                         "64 MB in all: a fixed, seeded sample of a larger output)")
    args = ap.parse_args()
    c_clips, c_fpc, c_nl, c_h, c_w, c_mode = CONFIGS[args.config]
    clips = args.clips if args.clips is not None else c_clips
    fpc = args.frames_per_clip if args.frames_per_clip is not None else c_fpc
    nl = args.layers if args.layers is not None else c_nl
    h = args.height if args.height is not None else c_h
    w = args.width if args.width is not None else c_w
    mode = args.mode or c_mode
    custom = (clips, fpc, nl, h, w, mode) != CONFIGS[args.config] or args.sigma != 0.05

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` with no launcher around it: start the N ranks ourselves.  Nothing has touched
        # the GPU yet (importing torch does not), so a CHILD process is safe; this process only waits, forwards the
        # child's output and exits with its code (never exec: the pool forbids replacing a process image).
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with "
                  f"python -m torch.distributed.run --nproc-per-node {args.gpus}", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print(f"bench.py: rank {rank} of {world} needs a GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        sys.exit(1)
    if args.dist_backend == "gloo":
        local_rank = local_rank % torch.cuda.device_count()  # ranks may share a GPU in the smoke test
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        from waldo_amd.dist import init_distributed
        init_distributed(backend=args.dist_backend)

    import waldo_amd
    from waldo_amd import _lib, functional as WF
    if args.lib:
        _lib.use_library(args.lib)
    for opt in args.debug_option:
        assert _lib.load().waldo_set_debug_option(opt, 1) == 0
    from waldo_amd.graphs import GraphedCall
    from waldo_amd.tools.utils import get_grid

    if args.config == "LVD":
        run_lvd(args, clips, world, rank, device, dist)
        return
    if args.config == "WIF":
        run_wif(args, clips, world, rank, device, dist)
        return
    if args.pipeline:
        if args.config not in ("C4", "C5"):
            print("bench.py: --pipeline runs the C4 / C5 recipes (only --clips may be overridden)", file=sys.stderr)
            sys.exit(2)
        run_pipeline(args, clips, world, rank, device, dist)
        return

    frames = clips * fpc
    tps = waldo_amd.TPSWarp(h, w, get_grid(4, 4).view(-1, 2)).to(device)
    layers, pts, occ = synth(frames, nl, h, w, device, seed=rank, sigma=args.sigma)
    if mode == "train":
        layers.requires_grad_()
        pts.requires_grad_()

    from waldo_amd.dist import all_gather_frames_async

    graphed = None
    pending = [None]  # the previous step's all-gather, still in flight while this step computes
    if mode == "fwd":  # launch-bound shapes: the call sequence replayed from one HIP graph
        graphed = GraphedCall(lambda l, p, o: WF.warp_composite(l, p, o, tps.inverse_kernel, tps.basis_t),
                              layers, pts, occ)

    def square_mean(rgb):  # the loss exactly as SURVEY 8(d) writes it: autograd's own gradient chain
        return rgb.square().mean()

    last = {}  # what the last step handed its caller (--dump-outputs)

    def step(loss=None):
        if mode == "fwd":
            with torch.no_grad():
                last["rgb"] = graphed(*graphed.inputs)  # the graph's own static buffers: no input copy in the step
            return
        if mode == "infer":
            with torch.no_grad():
                rgb = WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)
                prev, pending[0] = pending[0], all_gather_frames_async(rgb, frames * world)
                if prev is not None:
                    prev.wait()
            last["rgb"] = rgb
            return
        layers.grad = None
        pts.grad = None
        rgb = WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)
        out = (loss or square_mean)(rgb)
        out.backward()
        last["rgb"], last["loss"] = rgb.detach(), out.detach()

    def fence():
        if pending[0] is not None:  # every gather started inside a timed region ends inside it
            pending[0].wait()
            pending[0] = None
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n, **kw):
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            step(**kw)
        fence()
        return time.perf_counter() - t0

    box = {"seed": rank}

    def fresh_inputs():
        nonlocal layers, pts, occ
        layers = pts = occ = None
        gc.collect()
        torch.cuda.empty_cache()
        box["seed"] += 1000
        layers, pts, occ = synth(frames, nl, h, w, device, seed=box["seed"], sigma=args.sigma)
        if mode == "train":
            layers.requires_grad_()
            pts.requires_grad_()
        for _ in range(3):
            step()

    for _ in range(3):  # (the interpreter settles first: its full collection is a pause of the launch queue)
        step()
    settle_interpreter()
    settle_ms = settle_gpu(step, fence)
    for _ in range(args.warmup):
        step()
    blocks = timed_blocks(step, fence, args.steps, dist, device, args.dist_backend, nblocks=timed_block_count(args),
                          between=fresh_inputs if args.fresh_inputs_per_block else None)
    elapsed = median_block(blocks)
    if args.dump_outputs and rank == 0:
        outputs = dict(last)
        if mode == "train":
            outputs.update(grad_layers=layers.grad, grad_pts=pts.grad)
        dump_outputs(args.dump_outputs, outputs)
    loss_variants = launch_split = None
    if args.full:
        # the same step with the loss gradient 2 * rgb / N written as ONE elementwise kernel (_SquareMean) instead of
        # autograd's four-pass chain: reported next to the headline, never as it
        if mode == "train" and world == 1:
            n = max(5, min(args.steps, 20))
            for _ in range(2):
                step(loss=_SquareMean.apply)
            one_pass = sorted(timed(n, loss=_SquareMean.apply) / n for _ in range(3))[1]
            loss_variants = {"autograd_loss_ms_per_step": round(elapsed / args.steps * 1e3, 4),
                             "one_pass_loss_gradient_ms_per_step": round(one_pass * 1e3, 4),
                             "note": "value / ms_per_step use out.square().mean().backward() as it is written in SURVEY "
                                     "8(d); the second line is the same step with the loss gradient 2*rgb/N in one "
                                     "elementwise pass (bench.py:_SquareMean, same numbers; median of 3 short blocks)"}
        # per-entry-point device times from a SEPARATE pass (event pairs on the launch stream around every C-ABI call):
        # the timed blocks above carry no events
        n_events = max(5, min(args.steps, 20))
        with _lib.KernelTimer() as kt:
            timed(n_events)

        # launch-bound shapes: what part of a replay is kernel, what part the floor of launching a graph
        if mode == "fwd" and world == 1:
            n = max(args.steps, 50)
            tiny = GraphedCall(lambda t: t.add_(1.0), torch.zeros(64, device=device))
            tiny(*tiny.inputs)
            fence()
            t0 = time.perf_counter()
            for _ in range(n):
                tiny(*tiny.inputs)
            fence()
            floor_us = (time.perf_counter() - t0) / n * 1e6
            reps_in_graph = 16
            many = GraphedCall(lambda l, p, o: [WF.warp_composite(l, p, o, tps.inverse_kernel, tps.basis_t)
                                                for _ in range(reps_in_graph)][-1], layers, pts, occ)
            many(*many.inputs)
            fence()
            t0 = time.perf_counter()
            for _ in range(n):
                many(*many.inputs)
            fence()
            many_us = (time.perf_counter() - t0) / n * 1e6
            kernel_us = (many_us - floor_us) / reps_in_graph
            alg_fwd = (16 * nl + 12) * h * w * frames
            launch_split = {"replay_us": round(elapsed / args.steps * 1e6, 2),
                            "empty_graph_replay_us": round(floor_us, 2),
                            "kernel_us": round(kernel_us, 2),
                            # the roofline fraction on either clock: a whole replay (what `roofline.frac` uses) and the
                            # kernel without the per-replay launch floor
                            "frac_replay": round(alg_fwd / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                            "frac_kernel": round(alg_fwd / (kernel_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                            "note": f"empty graph = one 64-element add; kernel_us = (replay of a graph of {reps_in_graph} "
                                    "forwards - empty-graph replay) / 16: the forward kernel with its in-graph dependency "
                                    "boundary, without the per-replay launch floor"}

    out = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        total_frames = frames * world
        value = total_frames / (elapsed / args.steps)
        hw = h * w
        roof = None
        if args.full:
            alg = {"waldo_warp_composite_fwd": (16 * nl + 12) * hw * frames,
                   "waldo_warp_composite_bwd": (32 * nl + 12) * hw * frames}
            if mode != "train":
                alg.pop("waldo_warp_composite_bwd")
            if mode == "fwd":
                # inside a graph the per-call events are not recorded: the replay time is the kernel
                # time plus the graph's launch floor
                ks = {"waldo_warp_composite_fwd": (args.steps, ms_per_step)}
            else:
                ks = kt.summary()  # (from the separate events pass)
                # without autograd the forward is the one-launch entry point from the control points
                # (same kernel, mapping folded in): reported under the forward's name
                if "waldo_warp_composite_pts_fwd" in ks and "waldo_warp_composite_fwd" not in ks:
                    ks["waldo_warp_composite_fwd"] = ks.pop("waldo_warp_composite_pts_fwd")
            dom = max(alg, key=lambda k: ks[k][1])
            kern = {}
            for k in alg:
                gbs = alg[k] / (ks[k][1] * 1e-3) / 1e9
                kern[k] = {"launches": ks[k][0], "ms": round(ks[k][1], 4), "alg_bytes": alg[k],
                           "GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4)}
            # HBM-side bytes per launch: measured by two rocprofv3 --pmc children of this very command (the default
            # workload on one GPU), else from the committed passes of the same command (profiles/traffic.json)
            live, live_note = None, None
            if args.config == "C3" and not custom and world == 1 and not args.no_live_traffic:
                try:
                    live = live_traffic(["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-live-traffic"])
                except Exception as exc:  # (the line stands on the committed passes)
                    live_note = f"live passes failed ({type(exc).__name__}: {str(exc)[:200]})"

            def moved_bytes(k):
                return live[k] if live and live.get(k) else measured_traffic(k, frames, nl, h, w)

            traffic = moved_bytes(dom)
            copy_gbs = copy_bandwidth(device)  # measured D2D copy rate of this box (read + write bytes per second)
            for k in kern:
                # next to the fraction of the 8 TB/s spec: the fraction of what a copy kernel reaches on THIS box, and
                # what the entry point really moved
                kern[k]["frac_of_copy"] = round(kern[k]["GBps"] / copy_gbs, 4)
                moved = moved_bytes(k)
                if moved:
                    kern[k]["moved_bytes"] = int(moved)
                    kern[k]["moved_over_alg"] = round(moved / alg[k], 3)
                    kern[k]["moved_GBps"] = round(moved / (kern[k]["ms"] * 1e-3) / 1e9, 1)
                    kern[k]["moved_frac_of_copy"] = round(kern[k]["moved_GBps"] / copy_gbs, 4)
            roof = {"bound": "hbm", "kernel": dom, "achieved": kern[dom]["GBps"], "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": kern[dom]["frac"], "traffic": traffic,
                    "traffic_source": (("rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE, two child runs of "
                                        "this command in this run (FETCH_SIZE x2: gfx950 tallies 128-byte requests at "
                                        "64 bytes; KiB -> bytes), mean per dispatch, summed over the entry point's "
                                        "kernels") if live else
                                       ("profiles/traffic.json: rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this "
                                        "workload, committed; not re-measured in this run"
                                        + (": " + live_note if live_note else "")))
                    if traffic else None,
                    "ms_per_launch": kern[dom]["ms"], "alg_bytes_per_launch": alg[dom],
                    "kernels": kern}
            roof["copy_GBps"] = round(copy_gbs, 1)
            roof["frac_of_copy"] = kern[dom]["frac_of_copy"]
            roof["guide_copy_GBps"] = 6290.0  # the MI355X float4 device-copy figure; measured boxes reach 4.7-5.1 TB/s
        what = {"train": "fwd+bwd", "infer": "fwd only + all-gather", "fwd": "fwd only (HIP-graph replay)"}[mode]
        if args.config == "C3" and not custom:
            metric = "warped+composited frames/sec at 256x512, 8 layers; fwd+bwd"
        else:
            metric = f"warped+composited frames/sec at {h}x{w}, {nl} layers; {what} (not the headline metric)"
        out = {
            "metric": metric,
            "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{'custom (from ' + args.config + ')' if custom else args.config}: "
                                   f"{clips} clips x {fpc} frames per GPU, "
                                   f"{nl} layers x 4x{h}x{w}, 16 TPS control points, {what}",
                       "frames_per_gpu": frames, "layers": nl, "height": h, "width": w,
                       "parallelism": f"frames sharded x{world}, "
                                      + ("one all-gather of the composited frames per step, overlapped with the next "
                                         "step's kernels" if mode == "infer"
                                         else "no data-path collective")},
        }
        if roof is not None:
            out["roofline"] = roof
        out.update(block_fields(blocks, args.steps, settle_ms))
        if loss_variants is not None:
            out["loss_variants"] = loss_variants
            out["value_one_pass_loss_gradient"] = round(
                total_frames / (loss_variants["one_pass_loss_gradient_ms_per_step"] * 1e-3), 2)
        if launch_split is not None:
            out["launch_split"] = launch_split
    # the north star's multi-GPU evidence rides on the default workload's --full line
    want_ns = args.north_star == "on" or (args.north_star == "auto" and args.full and world > 1 and args.config == "C3"
                                           and not custom)
    if want_ns and dist is not None:
        del layers, pts, occ
        torch.cuda.empty_cache()
        if rank == 0:  # (a copy on stderr first: should the block take the process down, the headline was said)
            print("bench.py: headline before the north_star block: " + json.dumps(out), file=sys.stderr, flush=True)
        ns = north_star_block(args, world, rank, device, dist)
        if rank == 0:
            out["north_star"] = ns
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(nl, h, w, min(args.cpu_frames, max(1, 28 * 131072 // hw)),
                                               args.cpu_reps)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def north_star_block(args, world, rank, device, dist):
    """What BASELINE.json's north star asks of N GPUs, measured by the ONE multi-GPU command the driver runs
    (`bench.py --gpus N`), after its headline loop -- every rank calls this; rank 0 gets the object for the line:

      all_gather     the C4 and C5 synthetic forwards with the all-gather of the composited frames (SURVEY 8e;
                     tools/engine.py:86-92 is the reference's all_gather): frames and bytes per rank, the collective
                     alone (ms, GB/s received per rank), the step with the gather waited for at once (overlap off) and
                     overlapped with the next step's kernels (overlap on), and what of it stays exposed in either form
      strong_split   the C5 pipeline (Synthesizer.predict's hot-path calls) as ONE job of 4 clips whose (b, t) output
                     units are dealt over the N ranks (tools/demo.py:predict_sharded), one all-gather of the predicted
                     frames per step: ms_per_step (max over ranks), every rank's own compute time, the whole job on rank 0
                     alone and the speed-up over it
      gather_bit_equal   a 1-clip job split over the ranks and all-gathered equals the single-rank predict() bit for bit
                     on EVERY rank (all-reduced)
      rccl_ranks     the world size the communicator reports, `backend` its name ("nccl" is RCCL on ROCm)

    A part that raises is recorded as a string; the headline and the exit code survive it."""
    import waldo_amd
    from waldo_amd import functional as WF
    from waldo_amd.dist import all_gather_frames, all_gather_frames_async
    from waldo_amd.tools.pipeline import Pipeline
    from waldo_amd.tools.utils import get_grid
    n = max(3, min(args.steps, 10))
    cpu_coll = args.dist_backend != "nccl"
    res = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(), "steps_per_measurement": n}

    def fence():
        dist.barrier()
        torch.cuda.synchronize()

    def timed_max(fn, wait=None):
        """ms per call of fn over n calls between fences, max over ranks."""
        fn()
        if wait is not None:
            wait()
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        if wait is not None:
            wait()
        fence()
        t = torch.tensor([(time.perf_counter() - t0) / n * 1e3], device="cpu" if cpu_coll else device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item()

    def gather_part(name):
        c_clips, c_fpc, c_nl, c_h, c_w, _ = CONFIGS[name]
        frames = c_clips * c_fpc
        tps = waldo_amd.TPSWarp(c_h, c_w, get_grid(4, 4).view(-1, 2)).to(device)
        layers, pts, occ = synth(frames, c_nl, c_h, c_w, device, seed=rank)
        pending = [None]

        def fwd():
            with torch.no_grad():
                return WF.warp_composite(layers, pts, occ, tps.inverse_kernel, tps.basis_t)

        rgb = fwd()

        def sync_step():
            all_gather_frames(fwd(), frames * world)

        def overlapped_step():
            prev, pending[0] = pending[0], all_gather_frames_async(fwd(), frames * world)
            if prev is not None:
                prev.wait()

        def drain():
            if pending[0] is not None:
                pending[0].wait()
                pending[0] = None

        kernel_ms = timed_max(fwd)
        gather_ms = timed_max(lambda: all_gather_frames(rgb, frames * world))
        off_ms = timed_max(sync_step)
        on_ms = timed_max(overlapped_step, wait=drain)
        nbytes = rgb.numel() * 4
        return {"workload": f"{name}: {frames} frames of {c_h}x{c_w}, {c_nl} layers per rank, forward + all-gather",
                "frames_per_rank": frames, "bytes_sent_per_rank": nbytes, "bytes_received_per_rank": nbytes * (world - 1),
                "forward_ms": round(kernel_ms, 4), "all_gather_alone_ms": round(gather_ms, 4),
                "all_gather_GBps_received_per_rank": round(nbytes * (world - 1) / (gather_ms * 1e-3) / 1e9, 2),
                "step_ms_overlap_off": round(off_ms, 4), "step_ms_overlap_on": round(on_ms, 4),
                "exposed_ms_overlap_off": round(off_ms - kernel_ms, 4), "exposed_ms_overlap_on": round(on_ms - kernel_ms, 4)}

    def strong_part():
        name = args.north_star_config
        clips = CONFIGS[name][0]
        pipe = Pipeline(name, clips, device, seed=0, motion=args.motion, shard=(rank, world))
        tp = pipe.frames - pipe.ctx_len
        pending = [None]

        def own():
            return pipe()["inp_pred_vid"]

        def step():
            prev, pending[0] = pending[0], all_gather_frames_async(own(), clips * tp)
            if prev is not None:
                prev.wait()

        def drain():
            if pending[0] is not None:
                pending[0].wait()
                pending[0] = None

        for _ in range(2):
            own()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            own()
        torch.cuda.synchronize()
        mine = torch.tensor([(time.perf_counter() - t0) / n * 1e3], device="cpu" if cpu_coll else device, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        job_ms = timed_max(step, wait=drain)
        whole_ms = None
        if rank == 0:  # the whole job on one GPU, the others idle: T(1) of the speed-up
            whole = Pipeline(name, clips, device, seed=0, motion=args.motion)
            for _ in range(2):
                whole()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                whole()
            torch.cuda.synchronize()
            whole_ms = (time.perf_counter() - t0) / n * 1e3
            del whole
        fence()
        per_rank = [round(x.item(), 4) for x in every]
        out = {"workload": f"{name} pipeline, ONE job of {clips} clips x {pipe.frames} frames split over {world} ranks by (b, t) "
                           f"output units, one all-gather of the inpainted predicted frames per step (overlapped)",
               "ms_per_step": round(job_ms, 4), "per_rank_compute_ms": per_rank,
               "rank_imbalance_max_over_min": round(max(per_rank) / max(min(per_rank), 1e-9), 3)}
        if rank == 0:
            out["whole_job_on_rank0_ms"] = round(whole_ms, 4)
            out["speedup_over_one_gpu"] = round(whole_ms / job_ms, 3)
            out["frames_per_s"] = round(clips * pipe.frames / (job_ms * 1e-3), 2)
        return out

    def equal_part():
        name = args.north_star_config
        one = Pipeline(name, 1, device, seed=0, motion=args.motion, shard=(rank, world))
        got = one.gather(one(phases=("pred",)), keys=["inp_pred_vid"])["inp_pred_vid"]
        ref = Pipeline(name, 1, device, seed=0, motion=args.motion)()["inp_pred_vid"]
        ok = torch.tensor([1 if torch.equal(got, ref) else 0], device="cpu" if cpu_coll else device, dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(ok.item())

    parts = (("all_gather_C4", lambda: gather_part("C4")), ("all_gather_C5", lambda: gather_part("C5")),
             ("strong_split", strong_part), ("gather_bit_equal", equal_part))
    for key, fn in parts:
        try:
            res[key] = fn()
        except Exception as exc:  # (recorded, not raised: the headline line and the exit code survive)
            res[key] = f"failed: {type(exc).__name__}: {exc}"
        torch.cuda.empty_cache()
    return res


def run_lvd(args, clips, world, rank, device, dist):
    """`--config LVD`: the warp-path part of one LVD training step at the reference's recipe (models/synthesizer.py:
    815-841, scripts/cityscapes/train_lvd.sh) -- forward, loss and backward through TPS grids, grid inversion,
    grid_to_flow, input_to_output -- with a per-entry-point table.  Clips are independent: ranks keep their own
    (DDP's split, tools/engine.py:63-64), no data-path collective; the networks whose gradients DDP would reduce
    are outside the path."""
    from waldo_amd import _lib
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(clips, device, seed=rank)

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    names = ("raw", "pose_o", "pose_b", "score", "cls_logit")  # step.leaves, in order
    last = {}

    def run():  # the step, keeping the loss it hands its caller (--dump-outputs); detached: a loss that kept the
        last["loss"] = step().detach()  # autograd graph alive would keep its AccumulateGrad nodes on this stream

    def dump():  # what the headline's last timed step computed: the loss and the leaves' gradients
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, dict(loss=last["loss"], **{"grad_" + n: x.grad
                                                                       for n, x in zip(names, step.leaves)}))

    for _ in range(3):  # (the interpreter settles first: its full collection is a pause of the launch queue)
        step()
    settle_interpreter()
    settle_ms = settle_gpu(step, fence)
    for _ in range(args.warmup):
        step()
    nblocks = timed_block_count(args)
    blocks_eager = None
    if args.full or not args.graph:
        blocks_eager = timed_blocks(run, fence, args.steps, dist, device, args.dist_backend, nblocks=nblocks)
        if not args.graph:
            dump()
    # forward, loss and backward captured ONCE and replayed (the library launches on the current stream and never
    # synchronises; the frame indices are validated by the kernels, in a replay as in an eager call).  The step is ~90
    # short launches behind ~1.6 ms of interpreter and autograd-engine time per step: eager, it runs at the speed of the
    # box's host; the replay is the GPU's time.  The leaves' gradients are the graph's buffers: every replay overwrites
    # them.  A capture that fails leaves the eager line standing (`--graph` then reports the failure as its ms_per_step
    # note); a hard GPU fault is not catchable in-process: the eager blocks above have been timed by then.
    blocks_graph, graph_note = None, None
    if args.full or args.graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graph_loss = step()
            settle_gpu(graph.replay, fence)
            blocks_graph = timed_blocks(graph.replay, fence, args.steps, dist, device, args.dist_backend,
                                        nblocks=nblocks)
            _lib.IndexStatus.check_all(sync=True)
            if args.graph:
                last["loss"] = graph_loss.detach()
                dump()
        except Exception as exc:
            graph_note = f"capture failed: {type(exc).__name__}: {exc}"
    if blocks_eager is None and blocks_graph is None:  # a plain --graph run whose capture failed: the eager line
        blocks_eager = timed_blocks(run, fence, args.steps, dist, device, args.dist_backend, nblocks=nblocks)
        dump()
    use_graph = args.graph and blocks_graph is not None
    blocks = blocks_graph if use_graph else blocks_eager
    elapsed = median_block(blocks)
    if args.full:
        elapsed_eager = median_block(blocks_eager)
        elapsed_graph = median_block(blocks_graph) if blocks_graph is not None else None
        grads_ok = step.grads_finite()
        # the per-entry-point table from a SECOND, untimed pass: a step is ~250 short launches queued ahead of the GPU,
        # and two event records around each of its ~70 library calls make the host the bottleneck (3.7 ms against 2.1)
        n_table = max(3, min(args.steps, 10))
        with _lib.KernelTimer() as kt:
            for _ in range(n_table):
                step()
            fence()
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        o, t = step.opt, step.frames
        h, w = o.dim, int(o.dim * o.aspect_ratio)
        out = {
            "metric": f"LVD training-step frames/sec through the warp path at {h}x{w}, {o.num_obj + 1} layers, "
                      f"{t}-frame clips; fwd+bwd (the reference's live backward path; not the headline metric)",
            "value": round(clips * t * world / (elapsed / args.steps), 2), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"LVD recipe step: {clips} clips x {t} frames per GPU, {o.num_obj} objects + background, "
                                   f"{step.num_lyt} layout classes, {h}x{w} with no full-resolution raster, ctx_mode prev + "
                                   f"include_self; decoder tail -> pose affine -> estimate_alpha_grid_occ -> decode_output "
                                   f"-> loss -> backward; the networks outside the path replaced by seeded leaves",
                       "frames_per_gpu": clips * t, "layers": o.num_obj + 1, "height": h, "width": w,
                       "parallelism": f"clips sharded x{world}, no data-path collective"},
        }
        if args.full:
            table = {}
            for name, (n, ms) in sorted(kt.summary().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                table[name] = {"launches_per_step": round(n / n_table, 2), "ms_per_step": round(n * ms / n_table, 4)}
            in_lib = sum(r["ms_per_step"] for r in table.values())
            dom = next(iter(table))
            out.update({
                "roofline": {"bound": "hbm", "kernel": dom, "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": None, "traffic": None,
                             "note": "a chain of ~35 latency- and atomics-bound launches on 63 MB of grids and 22 MB of "
                                     "alphas: no single kernel's algorithmic bytes describe it; per-kernel counters in "
                                     "profiles/r04_lvd_step_counters.txt", "ms_per_launch": table[dom]["ms_per_step"]},
                "pipeline": {"ms_in_library_calls": round(in_lib, 4), "ms_outside": round(ms_per_step - in_lib, 4),
                             "note": "per C-ABI entry point, event pairs on the launch stream, from a second untimed "
                                     "pass; ms_outside = autograd's own kernels (gradient accumulation, fills, the loss) "
                                     "and launch gaps",
                             "entry_points": table},
                "grads_finite": grads_ok})
        out["launch"] = ("the whole step (forward, loss, backward) replayed from one HIP graph" if use_graph
                         else "eager" + (f" ({graph_note})" if args.graph and graph_note else ""))
        if args.full:
            out["ms_per_step_eager"] = round(elapsed_eager / args.steps * 1e3, 4)
            out["ms_per_step_graph_replay"] = (round(elapsed_graph / args.steps * 1e3, 4) if elapsed_graph is not None
                                               else graph_note)
        out.update(block_fields(blocks, args.steps, settle_ms))
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_wif(args, clips, world, rank, device, dist):
    """`--config WIF`: BASELINE config 3 as the reference RUNS it -- the call order of Synthesizer.inpaint
    (models/synthesizer.py:517-576, 631-633) at the scripts/cityscapes/train_wif.sh recipe: under no_grad the
    producers, estimate_alpha_grid_occ and decode_output through the UNRESTRICTED Warper.grid_to_flow
    (models/nets/lvd.py:602-705: train_wif.sh does not pass --s_restrict_to_ctx) and input_to_output, then WIF.forward
    (models/nets/wif.py:37-57) with autograd, the L1 loss and its backward through waldo_wif_fuse_bwd
    (waldo_amd/tools/wif_step.py; the UNet's place is taken by a 1 x 1 convolution that carries gradients).  Clips are
    independent: ranks keep their own (DDP's split, tools/engine.py:63-64); the gradient all-reduce DDP would do is the
    stand-in network's, outside the path: no data-path collective."""
    from waldo_amd import _lib
    from waldo_amd.tools.wif_step import WifStep
    step = WifStep(clips, device, seed=rank, motion=args.motion)

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    last = {}

    def run():  # the step, keeping the loss it hands its caller (--dump-outputs); detached: a loss that kept the
        last["loss"] = step().detach()  # autograd graph alive would keep its AccumulateGrad nodes on this stream

    for _ in range(3):  # (the interpreter settles first: its full collection is a pause of the launch queue)
        step()
    settle_interpreter()
    settle_ms = settle_gpu(step, fence)
    for _ in range(args.warmup):
        step()
    blocks = timed_blocks(run, fence, args.steps, dist, device, args.dist_backend, nblocks=timed_block_count(args))
    elapsed = median_block(blocks)
    if args.dump_outputs and rank == 0:  # the loss, the stand-in network's gradients and the decode WIF fused
        outputs = {"loss": last["loss"], "raw_output": step.raw_output}
        outputs.update({"grad_unet_" + n.replace(".", "_"): p.grad for n, p in step.unet.named_parameters()})
        dump_outputs(args.dump_outputs, outputs)
    step.warper.check_time_indices()
    if args.full:
        # the no-grad half alone (what `inpaint` computes before net_ii): its share of the step
        decode_blocks = timed_blocks(step.decode, fence, max(3, args.steps // 2), dist, device, args.dist_backend,
                                     nblocks=3)
        decode_ms = median_block(decode_blocks) / max(3, args.steps // 2) * 1e3
        grads_ok = step.grads_finite()
        n_table = max(3, min(args.steps, 10))
        with _lib.KernelTimer() as kt:
            for _ in range(n_table):
                step()
            fence()
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        o, t = step.opt, step.frames
        hd, wd = step.vid.shape[-2:]
        out = {
            "metric": f"WIF training-step frames/sec at {hd}x{wd}, {o.num_obj + 1} layers, {t}-frame clips ({step.ctx_len} "
                      f"context + {t - step.ctx_len} predicted); warp path forward under no_grad + WIF.forward/backward, as "
                      f"Synthesizer.inpaint runs it (not the headline metric)",
            "value": round(clips * t * world / (elapsed / args.steps), 2), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"WIF recipe step (scripts/cityscapes/train_wif.sh: 8 clips over 4 GPUs): {clips} clips x {t} "
                                   f"frames per GPU, {o.num_obj} objects + background, {o.num_lyt} layout classes, layers at "
                                   f"{o.dim}x{int(o.dim * o.aspect_ratio)}, frames at {hd}x{wd}; no_grad: decoder tail -> pose "
                                   f"affine -> estimate_alpha_grid_occ -> cat(vid, lyt) -> decode_output (UNRESTRICTED "
                                   f"grid_to_flow + input_to_output); autograd: WIF.forward -> L1 loss -> backward; networks "
                                   f"outside the path replaced by seeded stand-ins (UNet: a 1x1 convolution 40 -> 5), "
                                   f"background motion '{args.motion}'",
                       "frames_per_gpu": clips * t, "layers": o.num_obj + 1, "height": hd, "width": wd,
                       "parallelism": f"clips sharded x{world}, no data-path collective"},
        }
        if args.full:
            alg = step.hd_algorithmic_bytes()
            table = {}
            for name, (n, ms) in sorted(kt.summary().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                per_step = n * ms / n_table
                row = {"launches_per_step": round(n / n_table, 2), "ms_per_step": round(per_step, 4)}
                if name in alg:
                    row["alg_bytes_per_step"] = alg[name]
                    row["GBps"] = round(alg[name] / (per_step * 1e-3) / 1e9, 1)
                    row["frac"] = round(row["GBps"] / HBM_PEAK_GBS, 4)
                table[name] = row
            in_lib = sum(r["ms_per_step"] for r in table.values())
            dom = max((k for k in alg if k in table), key=lambda k: table[k]["ms_per_step"])
            out.update({
                "roofline": {"bound": "hbm", "kernel": dom, "achieved": table[dom]["GBps"], "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": table[dom]["frac"], "traffic": None,
                             "alg_bytes_per_launch": alg[dom], "ms_per_launch": table[dom]["ms_per_step"]},
                "pipeline": {"ms_in_library_calls": round(in_lib, 4), "ms_outside": round(ms_per_step - in_lib, 4),
                             "ms_no_grad_decode": round(decode_ms, 4),
                             "note": "per C-ABI entry point, event pairs on the launch stream, from a second untimed "
                                     "pass; ms_outside = framework kernels (the cat of frames and layouts, the stand-in "
                                     "convolution forward + weight gradient, the loss) and launch gaps; "
                                     "ms_no_grad_decode = the step's first half alone (everything before net_ii)",
                             "entry_points": table},
                "grads_finite": grads_ok})
        out.update(block_fields(blocks, args.steps, settle_ms))
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_pipeline(args, clips, world, rank, device, dist):
    """BASELINE configs C4 / C5 as the reference runs them (models/synthesizer.py:434-472).

    weak scaling (default): every rank keeps `clips` whole clips of its own (clips are independent: no data-path
    collective until the end), runs predict() on them and the ranks all-gather the inpainted predicted frames.
    strong scaling (--scaling strong): the `clips` clips are ONE job; its (b, t) output frames are dealt over the
    ranks in contiguous blocks (predict_sharded: the context frames and what is computed from them replicated per
    rank, no collective inside), and ONE all-gather of the inpainted predicted frames ends the step."""
    from waldo_amd import _lib
    from waldo_amd.dist import all_gather_frames_async
    from waldo_amd.tools.pipeline import Pipeline
    strong = args.scaling == "strong"
    shard = None
    emulated = None
    if strong:
        shard = (rank, world)
        if args.shard:
            if world != 1:
                print("bench.py: --shard R/W emulates one rank of a W-rank job on ONE GPU", file=sys.stderr)
                sys.exit(2)
            emulated = tuple(int(x) for x in args.shard.split("/"))
            shard = emulated
    pipe = Pipeline(args.config, clips, device, seed=0 if strong else rank, motion=args.motion, shard=shard)
    t, hd, wd = pipe.frames, pipe.vid.shape[-2], pipe.vid.shape[-1]
    tp = t - pipe.ctx_len
    pending = [None]  # the previous step's all-gather: over xGMI while this step's kernels run

    graph_box = [pipe.graphed() if args.graph else None]
    last = {}  # what the last step handed its caller: this rank's inpainted predicted frames (--dump-outputs)

    def step():
        graph = graph_box[0]
        if graph is not None:
            out = graph(*graph.inputs)
            if dist is not None:
                out = out.clone()  # the graph's static buffer: the next replay overwrites it while the gather runs
        else:
            out = pipe()["inp_pred_vid"]
        last["inp_pred_vid"] = out
        if strong:  # out: this rank's block of the B * Tp predicted frames
            if emulated is not None:
                return
            prev, pending[0] = pending[0], all_gather_frames_async(out, clips * tp)
        else:
            prev, pending[0] = pending[0], all_gather_frames_async(out.reshape(clips * t, 3, hd, wd), clips * t * world)
        if prev is not None:
            prev.wait()

    def fence():
        if pending[0] is not None:  # every gather started inside the timed region ends inside it
            pending[0].wait()
            pending[0] = None
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(3):  # (the interpreter settles first: its full collection is a pause of the launch queue)
        step()
    settle_interpreter()
    settle_ms = settle_gpu(step, fence)
    for _ in range(args.warmup):
        step()
    blocks = timed_blocks(step, fence, args.steps, dist, device, args.dist_backend, nblocks=timed_block_count(args))
    elapsed = median_block(blocks)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(last))
    graph_ms = None
    if args.full:
        # one GPU, eager line: the same step replayed from ONE HIP graph beside it (the GPU's time without the launch
        # gaps; what `--graph` makes the line's ms_per_step)
        if dist is None and graph_box[0] is None and emulated is None:
            try:
                graph_box[0] = pipe.graphed()
                for _ in range(max(args.warmup, 1)):
                    step()
                gb = timed_blocks(step, fence, args.steps, nblocks=3)  # (the same step, its hand-over of the frames included)
                graph_ms = round(median_block(gb) / args.steps * 1e3, 4)
            except Exception as exc:  # (the eager line stands on its own)
                graph_ms = f"capture failed: {exc}"
            graph_box[0] = None
        # the per-entry-point table from a SEPARATE pass (event pairs around every C-ABI call; none inside a HIP graph)
        n_table = max(3, min(args.steps, 10))
        with _lib.KernelTimer() as kt:
            for _ in range(n_table):
                step()
            fence()
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        o = pipe.opt
        if args.full:
            table = {}
            alg = {} if strong else pipe.hd_algorithmic_bytes()  # (a rank's share of a split job: no per-kernel roofline)
            for name, (n, ms) in sorted(kt.summary().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                per_step = n * ms / n_table
                row = {"launches_per_step": round(n / n_table, 2), "ms_per_step": round(per_step, 4)}
                if name in alg:
                    row["alg_bytes_per_step"] = alg[name]
                    row["GBps"] = round(alg[name] / (per_step * 1e-3) / 1e9, 1)
                    row["frac"] = round(row["GBps"] / HBM_PEAK_GBS, 4)
                table[name] = row
            in_lib = sum(r["ms_per_step"] for r in table.values())
            if strong or not table:  # (inside a HIP graph the per-call events are not recorded: no table)
                dom = max(table, key=lambda k: table[k]["ms_per_step"]) if table else None
                roof = {"bound": "hbm", "kernel": dom, "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                        "traffic": None, "ms_per_launch": table[dom]["ms_per_step"] if table else None,
                        "note": ("rank 0's share of a split job; the per-kernel roofline of the whole job is the weak-scaling "
                                 "line's (same kernels, same shapes per unit)") if strong else
                                "replayed from one HIP graph: no per-call events; the eager line has the per-kernel table"}
            else:
                dom = max((k for k in alg if k in table), key=lambda k: table[k]["ms_per_step"])
                roof = {"bound": "hbm", "kernel": dom, "achieved": table[dom]["GBps"], "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": table[dom]["frac"], "traffic": None,
                        "alg_bytes_per_launch": alg[dom], "ms_per_launch": table[dom]["ms_per_step"]}
        if strong:
            u0, u1 = pipe.local_units("pred")
            r0, r1 = pipe.local_units("rec")
            total_frames = clips * t
            workload = (f"{args.config} pipeline, ONE job of {clips} clips x {t} frames ({pipe.ctx_len} context) split over "
                        f"{emulated[1] if emulated else world} ranks by (b, t) output units: rank "
                        f"{emulated[0] if emulated else 0} reconstructs units [{r0}, {r1}) of {clips * t} and predicts "
                        f"[{u0}, {u1}) of {clips * tp}")
            par = (f"(b, t) units sharded x{emulated[1] if emulated else world}, context frames and their grids / "
                   f"composited alphas replicated, "
                   + ("the step replayed from one HIP graph, " if args.graph else "")
                   + ("NO collective (one emulated rank on one GPU)" if emulated else
                      "one all-gather of the inpainted predicted frames per step, overlapped with the next step's kernels"))
        else:
            total_frames = clips * t * world
            workload = f"{args.config} pipeline: {clips} clips x {t} frames per GPU ({pipe.ctx_len} context)"
            par = (f"clips sharded x{world}, one all-gather of the inpainted predicted frames per step, "
                   f"overlapped with the next step's kernels")
        out = {
            "metric": f"WIF inference frames/sec at {hd}x{wd}, {o.num_obj + 1} layers, {t}-frame clips; full "
                      f"LVD->FLP->WIF pipeline around the hot path (not the headline metric)",
            "value": round(total_frames / (elapsed / args.steps), 2), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload + f", layers at {o.dim}x{int(o.dim * o.aspect_ratio)}, frames at {hd}x{wd}, "
                                   f"{o.num_obj} objects + background, {o.num_lyt} layout classes; "
                                   f"Synthesizer.predict's call order: reconstruction of all {t} frames and prediction "
                                   f"of the last {tp}; networks outside the path replaced by seeded "
                                   f"stand-ins (UNet stand-in costs nothing), background motion '{pipe.motion}'; what the two "
                                   f"decodes compute from the context alone runs once per step; `alpha` (2a'-1 of the context "
                                   f"frames, read by net_ii.inpaint with an inpainter only) is "
                                   f"{'written' if getattr(o, 'use_inpainter', False) else 'NOT produced (use_inpainter off)'}",
                       "frames_per_gpu": clips * t if not strong else round(clips * t / (emulated[1] if emulated else world), 2),
                       "layers": o.num_obj + 1, "height": hd, "width": wd, "parallelism": par},
        }
        if args.full:
            out["roofline"] = roof
            out["pipeline"] = {"ms_in_library_calls": round(in_lib, 4),
                               "ms_outside": round(ms_per_step - in_lib, 4),
                               "note": "per C-ABI entry point, event pairs on the launch stream, from a separate "
                                       "untimed pass; ms_outside = framework kernels and launch gaps between the "
                                       "calls (indexing, permutes, the stand-ins)",
                               "entry_points": table}
        out.update(block_fields(blocks, args.steps, settle_ms))
        if graph_ms is not None:
            out["ms_per_step_graph_replay"] = graph_ms
        if emulated:
            out["emulated_shard"] = {"rank": emulated[0], "world": emulated[1],
                                     "note": "value = the WHOLE job's frames / this one rank's step time: what the "
                                             "job would reach if every rank took this long and the gather were free"}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
