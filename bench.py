#!/usr/bin/env python3
"""bench.py — SpMM GFLOP/s (= 2*nnz*N/t) and achieved HBM GB/s against the roofline.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is ONE launch of the hot path (C = A @ B, valued CSR x dense fp32) over one resident batch of
synthetic input — what the reference's driver times 200x per width (spmm_test.cu:754-762).

A plain run does what the headline figure needs and nothing else: it generates the seeded operands, makes the
plan once, warms up (the 200 launches of the full run's per-launch statistic run untimed, then the W warm-up
steps, so that both modes start the timed region alike), times the K steps and prints the line (`value`, `ms_per_step` and the roofline priced with
the timed region). `--full` adds every side measurement and check described below: the median of per-launch
event pairs, the plan timed three times, the copy-rate yardstick and the ceilings it prices, the sampled-row
check against the CPU oracle, the other widths, graphs and configurations, the driver and reference-kernel legs,
and the CPU baselines (`--no-extra` / `--no-cpu-baseline` trim a `--full` run). `--dump-outputs DIR` writes, after
the timed steps, what the last step handed its caller (C, or a fixed seeded sample of its rows) as .npy files.

One GPU (the BENCH line): BASELINE.json configs[1], the com-Amazon-shaped graph (M = K = 334 863,
nnz = 1 851 744) at feature width 128 as a seeded synthetic stand-in (no network: SURVEY.md §8 d4) — since round 3
the planted-community stand-in `com-amazon-sbm` (clustering coefficient 0.408 against SNAP com-Amazon's 0.397, vertex ids
shuffled); rounds 1-2's structureless `com-amazon-like` (clustering 4e-5) is measured beside it in `extra` with the
same fields, so both series continue. Launches go
through a gespmm plan (the analysis stage: row clustering + task table, built ONCE outside the timed region, its
time reported as `plan_ms`; the plain entry point is timed beside it in `extra`). Inputs are resident in HBM
before the timed region. `roofline.kernel_us` is the AVERAGE launch duration over the timed region: one pair of HIP
events on the launch stream around the K steps, divided by K (what rocprofv3's per-kernel average of the same command
agrees with to ~1 %); `roofline.kernel_us_median_of_pairs` is the statistic of every OTHER entry of the record: the
median over event pairs around ten launches each (one launch each from 300 us up), >= 200 launches whatever --steps is —
a pair around every single launch, the statistic of rounds 2-4, reads ~3 us higher: the event handling between launches
is in it.

Several GPUs (the SCALE lines, one process per GPU): the north_star's experiment — ONE RMAT graph (Graph500
parameters; scale 26 = 2^30 edges unless --rmat-scale says otherwise) cut into nnz-balanced contiguous row shards
(strong scaling), dense width 256. Every rank generates its shard of A and its K/world rows of B; B is replicated by
RCCL all-gather (no reduction anywhere: output rows are independent). `value` is the kernel-only rate with the
replicated B resident, like the one-GPU line; `exchange` carries the end-to-end figures: the column-panel pipeline
(all-gather of panel p+1 on a second stream while panel p is multiplied) with the exchange INSIDE the timed region,
and the rate amortised over L uses of the same B.

The JSON line also carries
  roofline      algorithmic bytes / median kernel duration, against 8 TB/s HBM; `traffic` = bytes per
                launch from the rocprofv3 PMC passes recorded in profiles/hbm_traffic.json for exactly this workload;
  cpu_baseline  the oracle's restatement of the reference's CPU loop (spmm_test.cu:595-605) timed on this box's
                host cores (rank 0, one GPU only), full pass of the bench workload; `others` = configs 1, 4 in full and
                >= 1 % row samples of the reddit- and products-shaped graphs.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
FP32_VALU_PEAK_TFLOPS = 157.3
MIN_KERNEL_SAMPLES = 200  # the reference times 200 launches (ITER, spmm_test.cu:714)
STEADY_STATE = 1000000    # expected_launches of a plan whose analysis always pays (kernel-quality figures: widths, sweeps)

COPY_RATE_GUIDE_GBS = 6290.0  # MI355X_MICROARCH.md:35 — measured copy rate of the chip; the sanity bound for the rate measured in the run
LINE_LIMIT = 4096  # the final stdout line stays below this; everything else goes to EXTRA_FILE (and to stderr)
EXTRA_FILE = os.path.join("profiles", "bench_extra_last.json")
DUMP_BYTES = 60 * 1000 * 1000  # --dump-outputs writes at most this much (C whole, or a seeded sample of its rows)


def self_launch_argv(n, argv):
    """argv of `python -m torch.distributed.run` for n local ranks running this file with the same flags."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def dump_outputs(dirname, C, seed=0):
    """--dump-outputs: the (M, N) fp32 product the timed path handed its caller in its last step, as DIR/C_sample.npy, and the
    rows it holds as DIR/C_sample_rows.npy (float64). All of C when it fits in DUMP_BYTES, else a fixed seeded sample of rows in
    ascending order — the same rows for the same arguments, so that two builds can be compared output for output."""
    import numpy as np
    import torch

    M, N = int(C.shape[0]), int(C.shape[1])
    keep = max(1, DUMP_BYTES // (4 * N + 8))
    rows = np.arange(M) if M <= keep else np.sort(np.random.RandomState(seed).choice(M, keep, replace=False))
    sample = C[torch.from_numpy(rows.astype(np.int64)).to(C.device)].cpu().numpy().astype(np.float32, copy=False)
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "C_sample.npy"), sample)
    np.save(os.path.join(dirname, "C_sample_rows.npy"), rows.astype(np.float64))


def _r(x, nd=4):
    """Numbers in the final line: 4 significant decimals are what the sources of these figures carry."""
    if isinstance(x, float):
        return float("%.*g" % (nd + 2, x))
    if isinstance(x, dict):
        return {k: _r(v, nd) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, nd) for v in x]
    return x


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(full):
    """The ONE stdout line (< LINE_LIMIT characters): the contract's fields, `roofline` and `cpu_baseline`, and the short
    headline-grade blocks; `extra`, long descriptions and per-width sweeps stay in the side file named by `extra_file`."""
    out = {k: _r(full.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                        "scaling", "vs_baseline", "dtype", "data")}
    cfg = full.get("config", {})
    out["config"] = {k: (v if not isinstance(v, str) else v[:200]) for k, v in cfg.items()
                     if k in ("workload", "rows_per_gpu", "nnz_per_gpu", "ncols", "partition", "stand_in", "kernel")}
    out["roofline"] = _pick(full.get("roofline", {}), (
        "bound", "achieved", "peak", "unit", "frac", "traffic", "l2_hit_rate", "algorithmic_bytes_per_launch", "kernel_us",
        "kernel_us_median_of_pairs", "launches", "ceiling_frac", "achieved_over_ceiling", "traffic_floor", "ceiling_note", "gather_GBs"))
    out["roofline"].setdefault("traffic", None)
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        c2 = _pick(cb, ("value", "unit", "cores", "kind", "sample"))
        if isinstance(cb.get("all_cores"), dict):
            c2["all_cores"] = _pick(cb["all_cores"], ("value", "cores"))
        out["cpu_baseline"] = c2
    else:
        out["cpu_baseline"] = None
    for k in ("verified_vs_oracle", "plan_ms", "plan_ms_first_creation", "init_ms", "value_incl_plan_over_200_launches",
              "value_incl_first_plan_over_200_launches", "stateless_auto_plan", "series", "widths",
              "reference_kernel", "other_configs", "exchange", "one_gpu_reference", "extra_file"):
        if full.get(k) is not None:
            out[k] = _r(full[k])
    def lean(x):  # the line carries numbers: no nulls, long explanations cut (the side file has them whole)
        if isinstance(x, dict):
            return {k: lean(v) for k, v in x.items() if v is not None}
        if isinstance(x, str) and len(x) > 110:
            return x[:107] + "..."
        return x

    keep_null = {k: out.get(k) for k in ("vs_baseline", "cpu_baseline") if out.get(k) is None}  # (contract keys stay, null or not)
    traffic_null = out["roofline"].get("traffic") is None
    out = lean(out)
    out.update(keep_null)
    if traffic_null:
        out["roofline"]["traffic"] = None
    line = json.dumps(out, separators=(",", ":"))
    for drop in ("other_configs", "widths", "reference_kernel", "one_gpu_reference", "exchange", "series"):  # never reached by today's fields: a guard
        if len(line) < LINE_LIMIT:
            break
        out.pop(drop, None)
        line = json.dumps(out, separators=(",", ":"))
    return line


def emit(full):
    """Full record -> EXTRA_FILE + stderr; compact line -> stdout (last line, the only one starting with '{')."""
    path = os.path.join(ROOT, EXTRA_FILE)
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1)
        full["extra_file"] = EXTRA_FILE
    except OSError as ex:
        full["extra_file"] = "not written: %s" % ex
    sys.stderr.write("bench.py full record: " + json.dumps(full) + "\n")
    sys.stderr.flush()
    print(compact_line(full))
    sys.stdout.flush()


def algorithmic_bytes(M, K, N, nnz, valued=True):
    """rowptr + colind (+ val) + B read once + C written once."""
    return 4 * (M + 1) + 4 * nnz + (4 * nnz if valued else 0) + 4 * K * N + 4 * M * N


def roof_gflops(M, K, N, nnz, valued=True):
    ab = algorithmic_bytes(M, K, N, nnz, valued)
    return min(2.0 * nnz * N / (ab / (HBM_PEAK_GBS * 1e9)) / 1e9, FP32_VALU_PEAK_TFLOPS * 1e3)


class BenchEnv:
    """What the measured code needs from its surroundings: the device, the process group, event timing, seeded operands, the
    sampled-row checker — and the PRODUCT itself (`make_plan` / `product`). main() builds it on a HIP device with the library as
    the product; tests/test_graphs_and_dist.py builds it on the host under gloo with its checker injected as the product, so that
    every N > 1 branch of run_rmat() (rank-local generation, equal / ragged B shards, the panel pipeline, the record) runs in the
    CPU suite before an 8-GPU node ever sees it. bench.py itself never supplies a host product."""

    def __init__(self, torch, dist, dev, world, rank, use_dist, variant=-1, product=None, make_plan=None, on_local_product=None):
        self.torch, self.dist, self.dev = torch, dist, torch.device(dev)
        self.world, self.rank, self.use_dist, self.variant = world, rank, use_dist, variant
        self.cuda = self.dev.type == "cuda"
        self._product, self._make_plan, self.on_local_product = product, make_plan, on_local_product
        self.injected_product = product  # handed to PanelPipeline (None = the HIP path)

    # ---- the product
    def make_plan(self, rowptr, colind, K, N, val):
        if self._make_plan is not None:
            return self._make_plan(rowptr, colind, K, N, val)
        if self._product is not None:
            return None
        from gespmm_amd import spmm

        return spmm.SpmmPlan(rowptr, colind, K, N, variant=self.variant, values=val, reorder=False)

    def product(self, rowptr, colind, val, B, out, plan=None):
        if self._product is not None:
            return self._product(rowptr, colind, val, B, out)
        from gespmm_amd import spmm

        return spmm.csr_spmm(rowptr, colind, val, B, variant=self.variant, out=out, plan=plan)

    # ---- device plumbing
    def device_sync(self):
        if self.cuda:
            self.torch.cuda.synchronize()

    def sync_all(self):
        self.device_sync()
        if self.use_dist:
            self.dist.barrier()
            self.device_sync()

    def empty_cache(self):
        if self.cuda:
            self.torch.cuda.empty_cache()

    def free_bytes(self):
        if self.cuda:
            return self.torch.cuda.mem_get_info(self.dev)[0]
        return 1 << 62

    def generator(self, seed):
        g = self.torch.Generator(device=self.dev)
        g.manual_seed(seed)
        return g

    def make_B(self, K, N, seed=None):
        torch = self.torch
        gB = self.generator(1000 + N if seed is None else seed)
        out = torch.empty((K, N), dtype=torch.float32, device=self.dev)
        step = max(1, (1 << 28) // max(N, 1))  # bounded int32 temporaries for the 64-GiB operands
        for r0 in range(0, K, step):
            r1 = min(K, r0 + step)
            # reference value set: float(r % 100 - 50) / 100 (spmm_test.cu:586-594)
            out[r0:r1] = (torch.randint(0, 100, (r1 - r0, N), generator=gB, device=self.dev, dtype=torch.int32) - 50).float() / 100
        return out

    def kernel_times_us(self, fn, n):
        """n launches timed by HIP events on the launch stream (the torch current stream IS the stream handed to the C ABI); returns
        one duration per event pair. A pair around EVERY launch puts ~3 us of event handling between launches (35 against rocprofv3's
        33 us on a 33 us kernel): launches shorter than 300 us are timed ten to a pair — at least 20 pairs — and each pair reports its
        average launch. (Host environment of the CPU suite: wall clock per call.)"""
        torch = self.torch
        n = max(int(n), 1)
        self.launches_per_event_pair = 1
        if not self.cuda:
            out = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                out.append((time.perf_counter() - t0) * 1e6)
            return out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        batch = 10 if e0.elapsed_time(e1) * 1e3 < 300.0 and n >= 10 else 1
        pairs = max(n // batch, 20) if batch > 1 else n
        self.launches_per_event_pair = batch
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(pairs)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(pairs)]
        torch.cuda.synchronize()
        for i in range(pairs):
            starts[i].record()
            for _ in range(batch):
                fn()
            ends[i].record()
        torch.cuda.synchronize()
        return [s.elapsed_time(e) * 1e3 / batch for s, e in zip(starts, ends)]

    def max_over_ranks(self, seconds):
        if not self.use_dist:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64, device=self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def timed_region(self, fn, steps, warmup):
        ev = None
        if self.cuda:  # one pair of HIP events around the K timed steps, on the launch stream (torch's current stream)
            ev = (self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True))
            # torch makes a HIP event at its first record: here, not inside the timed window (a process that has timed nothing
            # before paid ~50 us for it inside the window: +2.5 us per step at --steps 20)
            ev[0].record()
            ev[1].record()
        for _ in range(warmup):
            fn()
        self.sync_all()
        t0 = time.perf_counter()
        if ev:
            ev[0].record()
        for _ in range(steps):
            fn()
        if ev:
            ev[1].record()
        self.sync_all()
        wall = time.perf_counter() - t0
        # average launch duration by the device's clock over the timed region (what roofline.achieved is priced with: event pairs
        # around EVERY launch — kernel_us_median_of_pairs — put ~3 us of event handling between launches, and rocprofv3 does not see that)
        self.region_event_us = ev[0].elapsed_time(ev[1]) * 1e3 / max(int(steps), 1) if ev else wall * 1e6 / max(int(steps), 1)
        return self.max_over_ranks(wall)

    def verify(self, rowptr, colind, val, B, C, nrows=512, tolerant=False):
        """Sampled rows against the CPU oracle (checker only, outside every timed region): bit for bit; with `tolerant`
        (matrices whose hub rows take the long-row pass, a re-association) rows that differ must be within
        1e-4 * max(|ref|, sum |a*b|) and the counts are reported."""
        torch, dev = self.torch, self.dev
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import numpy as np

        import oracle_py

        M = rowptr.numel() - 1
        rng = np.random.RandomState(0)
        rows = np.sort(rng.choice(M, min(nrows, M), replace=False))
        rph = rowptr.cpu().numpy()
        sub_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
        sub_ptr[1:] = np.cumsum(rph[rows + 1] - rph[rows])
        sel = torch.from_numpy(np.concatenate([np.arange(rph[r], rph[r + 1]) for r in rows]).astype(np.int64)).to(dev)
        cih = colind[sel].cpu().numpy()
        vh = val[sel].cpu().numpy() if val is not None else None
        cols_u, inv = np.unique(cih, return_inverse=True)  # only the B rows these CSR rows touch travel to the host
        Bsub = B[torch.from_numpy(cols_u.astype(np.int64)).to(dev)].cpu().numpy()
        ref = oracle_py.spmm(sub_ptr, inv.astype(np.int32), vh, Bsub, "fma")
        got = C[torch.from_numpy(rows).to(dev)].cpu().numpy()
        same = (got.view(np.uint32) == ref.view(np.uint32)).all(axis=1)
        if not tolerant:
            return bool(same.all())
        scale = oracle_py.spmm_abs(sub_ptr, inv.astype(np.int32), vh, Bsub)
        close = (np.abs(got - ref) <= 1e-4 * np.maximum(np.abs(ref), scale) + 1e-12).all(axis=1)
        return {"rows": int(len(rows)), "bit_exact": int(same.sum()), "within_1e-4": int((close & ~same).sum()),
                "failed": int((~close).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ncols", type=int, default=0, help="feature width (default: 128 on one GPU, 256 for the RMAT run)")
    ap.add_argument("--graph", default=None,
                    help="named stand-in (default on one GPU: com-amazon-sbm) or 'rmat' (default on several GPUs)")
    ap.add_argument("--rmat-scale", type=int, default=0, help="log2(vertices) of the RMAT graph (default 26, the north_star's)")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--variant", type=int, default=-1)
    ap.add_argument("--locality", type=float, default=0.0, help="fraction of id-local edges in the stand-in")
    ap.add_argument("--no-plan", action="store_true", help="time the plain entry point as the headline")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and check (per-launch statistics, plan timing, copy rate and ceilings, "
                         "oracle check, other widths / graphs / configurations, driver and reference legs, CPU baselines)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/*.npy (at most 64 MB)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the side measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--panel-cols", type=int, default=128, help="column panel of the exchange/compute pipeline")
    ap.add_argument("--expected-launches", type=int, default=0,
                    help="expected_launches of the headline plan (0 = the library's default, 200 = the reference's protocol)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend of the several-GPU run (nccl = RCCL on ROCm)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run ... bench.py --gpus N ...` as a child
        # (one process per GPU; rendezvous on 127.0.0.1, a free port) — the line the ranks print is the same either way. This
        # process has not touched the device (nothing above imports torch or the library).
        import subprocess

        raise SystemExit(subprocess.call(self_launch_argv(args.gpus, sys.argv[1:])))

    import torch
    import torch.distributed as dist

    import gespmm_amd  # noqa: F401
    from gespmm_amd import _lib, graphs, spmm

    # this run creates products-sized plans several times in a row: keep their ~10 GB analysis arena between them (the library's
    # default keeps 1 GiB; a multi-GB hipMalloc was seen to take seconds now and then: profiles/r03/plan_repeat.log)
    _lib.set_cached_memory_limit(16 << 30)

    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d under a launcher with WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: there is no CPU path to measure")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or "RANK" in os.environ  # torchrun with 1 process still exercises RCCL
    if use_dist:
        dist.init_process_group(args.backend, **({"device_id": dev} if args.backend == "nccl" else {}))

    graph = args.graph or ("rmat" if world > 1 else "com-amazon-sbm")
    strong = graph == "rmat"
    N = args.ncols or (256 if strong else 128)

    # the library's warm-up, outside every timed region like the reference driver's 200 empty launches (spmm_test.cu:720-721): analysis
    # kernels loaded, analysis arena made (gespmm.h: gespmm_init). Without it the FIRST plan of a process costs ~36 ms instead of ~4
    # (profiles/r06/plan_cold.log) — under the reference's one-process-per-matrix protocol that decides whether a plan pays at all.
    torch.cuda.synchronize()
    t_init0 = time.perf_counter()
    _lib.init(400000, 2000000)
    _lib._initialised.add(local_rank)
    torch.cuda.synchronize()
    init_ms = (time.perf_counter() - t_init0) * 1e3

    env = BenchEnv(torch, dist, dev, world, rank, use_dist, variant=args.variant)
    sync_all, make_B, kernel_times_us, timed_region, verify = env.sync_all, env.make_B, env.kernel_times_us, env.timed_region, env.verify

    def measure_graph(g, val, N, valued=True, use_plan=True, samples=MIN_KERNEL_SAMPLES, keep=False, expected_launches=0, plan_reps=3):
        """Median kernel time of one (graph, width) through a plan (or the plain entry point). `expected_launches` goes to the plan:
        0 = the library's default, 200 (the reference's protocol) — an AUTO plan then skips an analysis that 200 launches would
        not pay for; STEADY_STATE = the kernel a long-running caller gets (what `widths` reports). The plain run's headline asks
        for samples = 0 and plan_reps = 1: operands, one plan and the step, nothing measured beside them."""
        M, K, nnz = g["M"], g["K"], g["nnz"]
        B = make_B(K, N)
        C = torch.empty((M, N), dtype=torch.float32, device=dev)
        v = val if valued else None
        plan, plan_ms, what = None, None, None
        plan_first_ms = None
        if use_plan:
            # the analysis stage (on the device): timed three times — the first creation in a process also pays for
            # loading the analysis kernels and growing the library's memory pool; `plan_ms` is the best of the other two
            times = []
            for _ in range(plan_reps):
                plan = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan = spmm.SpmmPlan(g["rowptr"], g["colind"], K, N, variant=args.variant, values=v, expected_launches=expected_launches)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            plan_first_ms, plan_ms = times[0], (min(times[1:]) if len(times) > 1 else None)
            what = plan.describe()

        def step():
            if valued:
                spmm.csr_spmm(g["rowptr"], g["colind"], v, B, variant=args.variant, out=C, plan=plan)
            else:
                spmm.csr_spmm_no_edge_value(g["rowptr"], g["colind"], B, variant=args.variant, out=C, plan=plan)

        for _ in range(5):
            step()
        if samples == 0:
            out = {"plan_ms_first_creation": plan_first_ms, "plan": what} if use_plan else {}
            return (out, step, B, C, plan) if keep else out
        us = kernel_times_us(step, samples)
        ab = algorithmic_bytes(M, K, N, nnz, valued)
        med = statistics.median(us)
        out = {"kernel_us": med, "kernel_us_mean": sum(us) / len(us), "kernel_us_min": min(us), "launches": len(us) * env.launches_per_event_pair,
               "launches_per_event_pair": env.launches_per_event_pair,
               "gflops": 2.0 * nnz * N / med / 1e3, "achieved_GBs": ab / med / 1e3, "frac": ab / med / 1e3 / HBM_PEAK_GBS,
               "roof_gflops": roof_gflops(M, K, N, nnz, valued)}
        if plan_ms is not None:
            out["plan_ms"] = plan_ms
            out["plan_ms_first_creation"] = plan_first_ms
            out["plan"] = what
            # the reference's own protocol is ITER = 200 launches per width (spmm_test.cu:714): rate with the analysis paid
            out["gflops_incl_plan_over_200_launches"] = 2.0 * nnz * N * 200 / (plan_ms * 1e3 + 200 * med) / 1e3
            out["gflops_incl_first_plan_over_200_launches"] = 2.0 * nnz * N * 200 / (plan_first_ms * 1e3 + 200 * med) / 1e3
            out["launches_to_amortise_plan_note"] = "plan_ms / (plain-call kernel_us - kernel_us); see plain_call_* beside this entry"
        if keep:
            return out, step, B, C, plan
        return out

    def measure_copy_rate():
        """Read + write rate of THIS box: the library's streaming-copy yardstick (gespmm_baseline_copy_f32) on 200 MB, 20 launches
        between one pair of events after 3 warm ones — outside every timed region. Bounded by the guide's figure."""
        n = 50 * 1000 * 1000
        src = torch.empty(n, dtype=torch.float32, device=dev).uniform_(-1, 1)
        dst = torch.empty_like(src)
        for _ in range(3):
            spmm.baseline_copy(src, out=dst)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            spmm.baseline_copy(src, out=dst)
        e1.record()
        torch.cuda.synchronize()
        ok = bool(torch.equal(src, dst))
        us = e0.elapsed_time(e1) * 1e3 / 20
        gbs = 8.0 * n / us / 1e3
        del src, dst
        how = "200 MB read + 200 MB written per launch, %.1f us, 20 launches%s" % (us, "" if ok else ", COPY WRONG")
        if gbs > 1.15 * COPY_RATE_GUIDE_GBS or gbs < 0.5 * COPY_RATE_GUIDE_GBS:  # a broken measurement must not price the ceiling
            return {"GBs": COPY_RATE_GUIDE_GBS, "how": "guide's figure (the run measured %.0f GB/s: out of the sanity range)" % gbs,
                    "measured_GBs": gbs}
        return {"GBs": gbs, "how": how, "measured_GBs": gbs}

    copy_rate = measure_copy_rate() if args.full and not strong else None  # (the several-GPU mode prices no ceiling)

    def ceiling_for(gx, n, frac):
        """Where the planted structure of a stand-in caps `frac`: inside a planted unit (perfect reuse inside, none across: the edges that
        leave it go to uniformly drawn rows) a B row is fetched ONCE if it can stay in the XCD's L2 while the unit is processed, C is
        written once, the CSR arrays read once — moved at the copy rate measured in this run. The unit is the coarsest planted level
        whose OWN rows of B fit an XCD's L2 at this width (3 MiB of the 4): the GROUP (com-Amazon-shaped: ~330 rows, products-shaped:
        ~1200), or the COMMUNITY where a group is larger than that (reddit-shaped: groups of 14 500 rows, communities of ~800).
        Round 6: the rows a unit REFERS to must fit as well — a reddit-shaped community refers to ~100 000 distinct rows (51 MB at
        N = 128) of which 3 MiB hold 6 144: the floor pins the unit's most referenced rows (fetched once) and charges every other
        reference as a fetch. Units whose references fit (the headline graph: ~550 rows per group) are priced as before."""
        if "truth_group" not in gx or copy_rate is None:
            return {}
        Mx, nz = gx["M"], gx["nnz"]
        lines_per_row = (4 * n + 127) // 128
        window_rows = (3 << 20) // (128 * lines_per_row)
        cache = gx.setdefault("_pairs", {})
        ngroups = int(gx["truth_group"].max()) + 1
        level = "group" if (Mx / max(ngroups, 1)) * 128 * lines_per_row <= (3 << 20) else "community"
        ck = (level, window_rows)
        if ck not in cache:
            rp = gx["rowptr"].long()
            unit = gx["truth_group"] if level == "group" else gx["truth_community"] + gx["truth_group"] * (int(gx["truth_community"].max()) + 1)
            keys = torch.repeat_interleave(unit.long(), rp[1:] - rp[:-1]) * gx["K"] + gx["colind"].long()
            uniq, cnt = torch.unique(keys, return_counts=True)
            del keys
            u = uniq // gx["K"]
            del uniq
            top = int(cnt.max())
            order = torch.argsort(u * (top + 1) + (top - cnt))  # by unit, most referenced rows first
            u, cnt = u[order], cnt[order]
            del order
            start = torch.zeros(int(u.max()) + 2, dtype=torch.long, device=u.device)
            start[1:] = torch.cumsum(torch.bincount(u), 0)
            rank = torch.arange(u.numel(), device=u.device) - start[u]
            pinned = rank < window_rows
            cache[ck] = (int(u.numel()), int(pinned.sum()) + int(cnt[~pinned].sum()))
            del u, cnt, rank, pinned, start
        pairs_all, pairs = cache[ck]
        floor = 128 * lines_per_row * pairs + 4 * Mx * n + 4 * (Mx + 1) + 8 * nz
        ab = algorithmic_bytes(Mx, gx["K"], n, nz, True)
        ceil = ab / (floor / copy_rate["GBs"]) / HBM_PEAK_GBS
        return {"traffic_floor": floor, "ceiling_frac": ceil, "achieved_over_ceiling": frac / ceil,
                "ceiling_note": "alg bytes / (traffic_floor / copy rate) / 8 TB/s; copy rate %.2f TB/s measured in this run (%s; the "
                                "guide's figure is %.2f); floor = B rows fetched per planted %s: its %d most referenced rows once, every other reference "
                                "once per use (%d fetches for %d distinct (unit, row) pairs) + C + CSR"
                                % (copy_rate["GBs"] / 1e3, copy_rate["how"], COPY_RATE_GUIDE_GBS / 1e3, level, window_rows, pairs, pairs_all)}

    pmc = {}
    pmc_path = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if os.path.exists(pmc_path):  # measured with rocprofv3 --pmc (separate passes), see profiles/README.md
        with open(pmc_path) as f:
            pmc = json.load(f)

    csrc_now = csrc_fingerprint()

    def traffic_for(key):
        """PMC figures recorded for this workload, or None when the kernel sources changed since they were captured
        (every entry carries the fingerprint of gespmm_amd/csrc at capture time: scripts/update_traffic_json.py)."""
        e = pmc.get(key)
        if not e:
            return None, None, None
        if e.get("csrc_sha16") != csrc_now:
            sys.stderr.write("bench.py: profiles/hbm_traffic.json[%s] was captured at csrc %s, the tree is at %s: "
                             "traffic not reported (re-capture: scripts/gpu_pmc.sh + scripts/update_traffic_json.py)\n" % (key, e.get("csrc_sha16"), csrc_now))
            return None, "stale: captured at csrc %s, tree at %s" % (e.get("csrc_sha16"), csrc_now), None
        return e.get("bytes_per_launch"), e.get("source"), e.get("l2_hit_rate")

    # =============================================================================================== several GPUs
    if strong:
        out = run_rmat(args, env, N, full=args.full)
        if rank == 0:
            emit(out)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    # =============================================================================================== one GPU (or replicas)
    g = graphs.synthetic_graph(graph, seed=42 + rank, device=dev, locality=args.locality)
    M, K, nnz = g["M"], g["K"], g["nnz"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(7 + rank)
    val = torch.rand(nnz, generator=gen, device=dev) - 0.5

    head, step, B, C, plan = measure_graph(g, val, N, True, use_plan=not args.no_plan, keep=True, expected_launches=args.expected_launches,
                                           samples=MIN_KERNEL_SAMPLES if args.full else 0, plan_reps=3 if args.full else 1)
    if not args.full:
        # the launches of the per-launch statistic a --full run takes here, untimed, so that both modes start the timed region from the
        # same device state (without them a region of 200 steps read 0.7 % slower, 0.0822 against 0.0815 ms per step; 5000 steps did not)
        for _ in range(MIN_KERNEL_SAMPLES):
            step()
    wall = timed_region(step, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, C)
    flop_per_step = 2.0 * nnz * N * world  # weak scaling: every rank owns one graph of this size
    value = flop_per_step * args.steps / wall / 1e9
    ms_per_step = wall / args.steps * 1e3
    verified = verify(g["rowptr"], g["colind"], val, B, C) if rank == 0 and args.full else None
    abytes = algorithmic_bytes(M, K, N, nnz, True)
    # the line's roofline is priced with the average launch duration over the timed region (HIP events around the K steps); the median
    # of per-launch event pairs (what the other entries of this record use: they are not timed as a region) stays beside it
    head["kernel_us_median_of_pairs"] = head.get("kernel_us")
    head["kernel_us"] = env.region_event_us
    head["achieved_GBs"] = abytes / head["kernel_us"] / 1e3
    head["frac"] = head["achieved_GBs"] / HBM_PEAK_GBS
    head["gflops"] = 2.0 * nnz * N / head["kernel_us"] / 1e3
    launch = "plan" if not args.no_plan else "plain"
    tkey = "%s/N%d/valued/%s" % (graph, N, launch)
    traffic, traffic_src, l2_hit = traffic_for(tkey) if (args.locality == 0.0 and world == 1) else (None, None, None)

    extra = {}
    series = {}   # headline-grade blocks that stay in the stdout line: the other com-Amazon stand-in (rounds 1-2's headline)
    widths = {}   # the metric's other widths on the headline graph
    reference_kernel = None
    stateless = None
    if args.full and not args.no_extra and world == 1:
        # the plain entry point on the same operands (what a caller without a plan gets; r01's headline)
        def plain():
            spmm.csr_spmm(g["rowptr"], g["colind"], val, B, variant=args.variant, out=C)

        for _ in range(5):
            plain()
        us = kernel_times_us(plain, MIN_KERNEL_SAMPLES)
        med = statistics.median(us)
        t2, s2, h2 = traffic_for("%s/N%d/valued/plain" % (graph, N))
        extra["plain_call_N%d_valued" % N] = {"kernel_us": med, "gflops": 2.0 * nnz * N / med / 1e3,
                                              "frac": abytes / med / 1e3 / HBM_PEAK_GBS, "traffic": t2, "l2_hit_rate": h2}
        widths["N%d_plain_call" % N] = {"kernel_us": med, "frac": abytes / med / 1e3 / HBM_PEAK_GBS}
        if plan is not None:  # the same plan after gespmm_plan_tune (kernel choice by measurement instead of by rule)
            t0 = time.perf_counter()
            plan.tune(B, out=C, reps=3)
            torch.cuda.synchronize()
            tune_ms = (time.perf_counter() - t0) * 1e3
            medt = statistics.median(kernel_times_us(step, MIN_KERNEL_SAMPLES))
            extra["headline_plan_after_tune"] = {"kernel_us": medt, "frac": abytes / medt / 1e3 / HBM_PEAK_GBS, "tune_ms": tune_ms,
                                                 "plan": plan.describe()}
        del B, C, plan
        for n2 in (32, 512):
            for valued in (True, False):
                torch.cuda.empty_cache()
                rw = measure_graph(g, val, n2, valued, samples=MIN_KERNEL_SAMPLES if valued else 50, expected_launches=STEADY_STATE)
                extra["N%d_%s" % (n2, "valued" if valued else "unweighted")] = rw
                if valued:
                    tw_, _, hw_ = traffic_for("%s/N%d/valued/plan" % (graph, n2))
                    widths["N%d" % n2] = {"kernel_us": rw["kernel_us"], "gflops": rw["gflops"], "frac": rw["frac"], "traffic": tw_,
                                          "l2_hit_rate": hw_}
                    widths["N%d" % n2].update({k: v for k, v in ceiling_for(g, n2, rw["frac"]).items()
                                               if k in ("ceiling_frac", "achieved_over_ceiling")})
        extra["N%d_unweighted" % N] = measure_graph(g, val, N, False, samples=50)
        # ---- round 6: feature widths that are not powers of two (100 / 200 features, 41 / 47 classes) through the
        #      general staged-rows kernel, and the max reducer through a plan
        for n2 in (100, 200, 47):
            torch.cuda.empty_cache()
            rw = measure_graph(g, val, n2, True, expected_launches=STEADY_STATE)
            rp2_ = measure_graph(g, val, n2, True, use_plan=False)
            extra["N%d_valued" % n2] = rw
            widths["N%d" % n2] = {"kernel_us": rw["kernel_us"], "frac": rw["frac"], "plain_call_kernel_us": rp2_["kernel_us"],
                                  "kernel": (rw.get("plan") or "").split("|")[-1].strip()[:24]}
        try:
            Bm = make_B(K, N)
            Cm = torch.empty((M, N), dtype=torch.float32, device=dev)
            pm = spmm.SpmmPlan(g["rowptr"], g["colind"], K, N, expected_launches=STEADY_STATE)
            want = spmm.csr_spmm_max(g["rowptr"], g["colind"], Bm)
            pm.run(None, Bm, out=Cm, reduce_max=-10000.0)
            t_max_plan = statistics.median(kernel_times_us(lambda: pm.run(None, Bm, out=Cm, reduce_max=-10000.0), 50))
            t_max_plain = statistics.median(kernel_times_us(lambda: spmm.csr_spmm_max(g["rowptr"], g["colind"], Bm), 50))
            extra["max_reducer_N%d" % N] = {"plan_kernel_us": t_max_plan, "plain_call_kernel_us": t_max_plain,
                                            "bits_equal_plain_call": bool(torch.equal(Cm.view(torch.int32), want.view(torch.int32))),
                                            "plan": pm.describe()}
            widths["N%d_max_reducer" % N] = {"kernel_us": t_max_plan, "plain_call_kernel_us": t_max_plain}
            del Bm, Cm, pm, want
        except Exception as ex:  # noqa: BLE001
            extra["max_reducer_N%d" % N] = {"skipped": "%s: %s" % (type(ex).__name__, str(ex)[:200])}
        # ---- round 6: the STATELESS entry points with gespmm_set_auto_plan (csrc/auto_plan.cpp): wall clock per call over 200 calls
        #      (the fingerprint's synchronisation is part of every call), DGL's argument list, unweighted; switch off / on
        try:
            import ctypes as _ct

            Bs = make_B(K, N)
            Cs = torch.empty((M, N), dtype=torch.float32, device=dev)
            P_ = lambda t: _ct.c_void_p(t.data_ptr())

            def dgl_call():
                _lib.check(_lib.lib.gespmm_dgl_csrmm_sum_f32(M, N, P_(g["rowptr"]), P_(g["colind"]), P_(Bs), P_(Cs), None), "dgl")

            def wall_us(fn, n=200):
                for _ in range(6):
                    fn()
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0_) / n * 1e6

            with torch.cuda.stream(torch.cuda.default_stream(dev)):
                _lib.set_auto_plan(0)
                off_us = wall_us(dgl_call)
                ref_s = Cs.clone()
                _lib.set_auto_plan(3)
                on_us = wall_us(dgl_call)
                same_s = bool(torch.equal(Cs.view(torch.int32), ref_s.view(torch.int32)))
                st_ = _lib.auto_plan_stats()
                _lib.set_auto_plan(0)
            stateless = {"entry": "gespmm_dgl_csrmm_sum_f32 N=%d" % N, "switch_off_us_per_call": off_us, "switch_on_us_per_call": on_us,
                         "bits_equal": same_s, "plans_created": st_["plans_created"]}
            del Bs, Cs, ref_s
        except Exception as ex:  # noqa: BLE001
            stateless = {"skipped": "%s: %s" % (type(ex).__name__, str(ex)[:200])}

        if graph in ("com-amazon-sbm", "com-amazon-like") and args.locality == 0.0:
            # ---- the OTHER com-Amazon stand-in, same M and nnz, same fields as the headline, so that every round has both:
            #      `com-amazon-sbm`  planted communities (SNAP: 75 149 communities, clustering 0.397; generated: 0.408), vertex
            #                        ids SHUFFLED — any locality is found by the plan's clustering, not inherited (headline
            #                        since round 3: it is the stand-in whose measured graph statistics match com-Amazon's);
            #      `com-amazon-like` structureless (clustering 4e-5: an expander; rounds 1-2's headline, the adversarial case)
            other = "com-amazon-like" if graph == "com-amazon-sbm" else "com-amazon-sbm"
            torch.cuda.empty_cache()
            gs = graphs.synthetic_graph(other, seed=42, device=dev)
            r = measure_graph(gs, val, N, True, expected_launches=STEADY_STATE)  # the clustered plan (the series of rounds 1-4)
            rdef = measure_graph(gs, val, N, True)  # ... and what a plan made with the defaults does: 200 expected launches
            r["default_policy_200_launches"] = {k: rdef.get(k) for k in ("kernel_us", "frac", "plan_ms", "gflops_incl_plan_over_200_launches", "plan")}
            r["traffic"], r["traffic_source"], r["l2_hit_rate"] = traffic_for("%s/N%d/valued/plan" % (other, N))
            rp_ = measure_graph(gs, val, N, True, use_plan=False, samples=MIN_KERNEL_SAMPLES)
            r["plain_call_kernel_us"] = rp_["kernel_us"]
            r["plain_call_gflops"] = rp_["gflops"]
            r["plain_call_frac"] = rp_["frac"]
            extra["%s_N%d_valued" % (other, N)] = r
            series[other] = {"kernel_us": r["kernel_us"], "gflops": r["gflops"], "frac": r["frac"], "traffic": r["traffic"],
                             "l2_hit_rate": r["l2_hit_rate"], "plan_ms": r.get("plan_ms"),
                             "plain_call_kernel_us": rp_["kernel_us"], "plain_call_frac": rp_["frac"],
                             "gflops_incl_plan_over_200_launches": r.get("gflops_incl_plan_over_200_launches"),
                             "default_plan_200_launches": {"kernel_us": rdef["kernel_us"], "plan_ms": rdef.get("plan_ms"),
                                                           "gflops_incl_plan": rdef.get("gflops_incl_plan_over_200_launches"),
                                                           "order": (rdef.get("plan") or "")[:13]}}
            series[other].update({k: v for k, v in ceiling_for(gs, N, r["frac"]).items() if k != "ceiling_note"})
            del gs
            # ---- round 6: the planted-community graph ARRIVING in its community order (rows and columns relabelled by the planted labels:
            #      a caller who keeps the graph that way). The plan keeps the caller's order; the fast kernels still apply
            try:
                torch.cuda.empty_cache()
                gp = graphs.synthetic_graph("com-amazon-sbm", seed=42, device=dev)
                rpp, cip = graphs.relabel_by_order(gp["rowptr"], gp["colind"], torch.argsort(gp["truth"]))
                gpo = {"M": gp["M"], "K": gp["K"], "nnz": gp["nnz"], "rowptr": rpp, "colind": cip}
                del gp
                arr = {}
                for n3 in (N, 32):
                    r3 = measure_graph(gpo, val, n3, True, expected_launches=STEADY_STATE)
                    p3 = measure_graph(gpo, val, n3, True, use_plan=False)
                    extra["com-amazon-sbm_planted_order_N%d_valued" % n3] = r3
                    arr["N%d" % n3] = {"kernel_us": r3["kernel_us"], "frac": r3["frac"], "plain_call_kernel_us": p3["kernel_us"],
                                       "plan": (r3.get("plan") or "")[:28] + " | " + (r3.get("plan") or "").split("|")[-1].strip()[:22]}
                series["com-amazon-sbm_arriving_in_planted_order"] = arr
                del gpo, rpp, cip
            except Exception as ex:  # noqa: BLE001
                series["com-amazon-sbm_arriving_in_planted_order"] = {"skipped": "%s: %s" % (type(ex).__name__, str(ex)[:160])}

            # ---- the second graph of BASELINE configs[1]: reddit-shaped x N=128 (cache-blocked path), sampled rows verified
            torch.cuda.empty_cache()
            g2 = graphs.synthetic_graph("reddit-like", seed=42, device=dev)
            val2 = torch.rand(g2["nnz"], device=dev) - 0.5
            r2, step2, B2, C2, plan2 = measure_graph(g2, val2, N, True, samples=10, keep=True)
            r2["verified_vs_oracle"] = verify(g2["rowptr"], g2["colind"], val2, B2, C2, nrows=128)
            r2["gather_GBs"] = 4.0 * g2["nnz"] * N / r2["kernel_us"] / 1e3
            r2["nnz"] = g2["nnz"]
            r2["note"] = "launch sequence of the cache-blocked path (one kernel per column slab; split points kept by the plan)"
            extra["reddit-like_N%d_valued" % N] = r2
            del g2, val2, B2, C2, plan2, step2

            # ---- the same shape WITH planted communities (the real reddit graph is made of subreddits; the stand-in above has no
            #      structure): AUTO plans analyse dense graphs too and keep the clustered order from 0.65 modelled L2 hits on
            torch.cuda.empty_cache()
            g2s = graphs.synthetic_graph("reddit-sbm", seed=42, device=dev)
            rpr, cir = g2s["rowptr"], g2s["colind"]
            val2s = torch.rand(g2s["nnz"], device=dev) - 0.5
            r2s, step2s, B2s, C2s, plan2s = measure_graph(g2s, val2s, N, True, samples=10, keep=True)
            r2s["verified_vs_oracle"] = verify(rpr, cir, val2s, B2s, C2s, nrows=128)
            r2s["plain_call_kernel_us"] = measure_graph(g2s, val2s, N, True, use_plan=False, samples=10)["kernel_us"]
            r2s["note"] = ("232 965 rows, 114.6 M entries, 290 planted communities (~800 rows, ~330 of a row's 492 entries inside), ids "
                          "shuffled: graphs.synthetic_graph('reddit-sbm')")
            r2s.update(ceiling_for(g2s, N, r2s["frac"]))
            extra["reddit-sbm_N%d_valued" % N] = r2s
            del g2s, val2s, B2s, C2s, plan2s, step2s, rpr, cir

            # ---- BASELINE configs[2]: products-shaped, N in {16..512}, the library's own choice per width — on the
            #      structureless stand-in and on the planted-community one (ids shuffled); ONE plan per graph (made for
            #      N = 128: the clustering does not depend on the width) serves the whole sweep
            for pname in ("products-like", "products-sbm"):
                torch.cuda.empty_cache()
                g3 = graphs.synthetic_graph(pname, seed=42, device=dev)
                val3 = torch.rand(g3["nnz"], device=dev) - 0.5
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan3 = spmm.SpmmPlan(g3["rowptr"], g3["colind"], g3["K"], 128, values=val3)
                torch.cuda.synchronize()
                sweep = {"plan_ms": (time.perf_counter() - t0) * 1e3, "plan": plan3.describe()}
                # (the staged-rows kernel's tables are made for ONE width: N = 32 / 64 — the lane-group form — and N = 256 / 512 get
                #  plans of their own)
                wide = {}
                for nw in (32, 64, 256, 512):
                    tw = []
                    for _ in range(2):
                        wide[nw] = None
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        wide[nw] = spmm.SpmmPlan(g3["rowptr"], g3["colind"], g3["K"], nw, values=val3)
                        torch.cuda.synchronize()
                        tw.append((time.perf_counter() - t0) * 1e3)
                    sweep["plan_N%d_ms" % nw] = min(tw)
                    sweep["plan_N%d_ms_each" % nw] = tw
                    sweep["plan_N%d" % nw] = wide[nw].describe()
                for n3 in (16, 32, 64, 128, 256, 512):
                    torch.cuda.empty_cache()
                    B3 = make_B(g3["K"], n3)
                    C3 = torch.empty((g3["M"], n3), dtype=torch.float32, device=dev)
                    ab3 = algorithmic_bytes(g3["M"], g3["K"], n3, g3["nnz"], True)
                    row = {"roof_gflops": roof_gflops(g3["M"], g3["K"], n3, g3["nnz"], True)}
                    for label, pl in (("plain", None), ("plan", wide.get(n3, plan3))):
                        def st3():
                            spmm.csr_spmm(g3["rowptr"], g3["colind"], val3, B3, variant=args.variant, out=C3, plan=pl)
                        for _ in range(2):
                            st3()
                        med3 = statistics.median(kernel_times_us(st3, 10))
                        row[label] = {"kernel_us": med3, "gflops": 2.0 * g3["nnz"] * n3 / med3 / 1e3,
                                      "achieved_GBs": ab3 / med3 / 1e3, "frac": ab3 / med3 / 1e3 / HBM_PEAK_GBS}
                    if pname == "products-sbm" and n3 in (128, 512):  # counters of this launch: scripts/gpu_profile_r04.sh
                        tb, tsrc, thit = traffic_for("products-sbm/N%d/valued/plan" % n3)
                        row["plan"].update({"traffic": tb, "traffic_source": tsrc, "l2_hit_rate": thit,
                                            "traffic_GBs": (tb / row["plan"]["kernel_us"] / 1e3) if tb else None,
                                            "algorithmic_bytes_per_launch": ab3})
                    row["plan"].update({k: v for k, v in ceiling_for(g3, n3, row["plan"]["frac"]).items() if k != "ceiling_note"})
                    sweep["N%d" % n3] = row
                    del B3, C3
                extra["%s_sweep_valued" % pname] = sweep
                del g3, val3, plan3, wide

            # ---- power-law graphs without communities (round-5 review: "the record should carry the power-law figures next to the
            #      headline"): Barabasi-Albert m = 6 and Holme-Kim m = 16 (the hold-out audit's networkx models, generated on the device:
            #      graphs.preferential_csr), N = 128, steady-state AUTO plan and the plain call
            for pname in ("ba-m6", "holme-kim-m16"):
                torch.cuda.empty_cache()
                gp_ = graphs.synthetic_graph(pname, seed=42, device=dev)
                vp_ = torch.rand(gp_["nnz"], device=dev) - 0.5
                rp_w = measure_graph(gp_, vp_, N, True, samples=50, expected_launches=STEADY_STATE)
                rp_w["plain_call_kernel_us"] = measure_graph(gp_, vp_, N, True, use_plan=False, samples=50)["kernel_us"]
                rp_w["nnz"], rp_w["rows"] = gp_["nnz"], gp_["M"]
                extra["powerlaw-%s_N%d_valued" % (pname, N)] = rp_w
                del gp_, vp_

            # ---- BASELINE configs[0] and [3]: the small graphs (launch-latency territory), unweighted as the reference's driver and
            #      its GCN run them; plain call and plan
            for sname, sN in (("cit-hepth-like", 32), ("pubmed-like", 128)):
                gsm = graphs.synthetic_graph(sname, seed=42, device=dev)
                vsm = torch.rand(gsm["nnz"], device=dev) - 0.5
                rs = measure_graph(gsm, vsm, sN, False, use_plan=True, samples=MIN_KERNEL_SAMPLES)
                rs["plain_call_kernel_us"] = measure_graph(gsm, vsm, sN, False, use_plan=False, samples=MIN_KERNEL_SAMPLES)["kernel_us"]
                extra["%s_N%d_unweighted" % (sname, sN)] = rs
                del gsm, vsm

            # ---- BASELINE configs[4] on ONE GPU through EXACTLY the path `--gpus N` runs (run_rmat, one rank, no
            #      process group): RMAT scale 26 x N = 256 when the device has the memory (MI355X: 137 GB of operands),
            #      else scale 24 — the same-workload one-GPU point a 2/4/8-GPU strong-scaling line is relative to
            torch.cuda.empty_cache()
            free_b, _ = torch.cuda.mem_get_info()
            rscale = 26 if free_b > (170 << 30) else 24
            rargs = argparse.Namespace(**vars(args))
            rargs.rmat_scale, rargs.steps, rargs.warmup, rargs.dump_outputs = rscale, 5, 2, None
            rline = run_rmat(rargs, BenchEnv(torch, dist, dev, 1, 0, False, variant=args.variant), 256,
                             with_cpu_baseline=not args.no_cpu_baseline)
            extra["rmat-%d_N256_valued" % rscale] = {
                "kernel_us": rline["roofline"]["kernel_us"], "ms_per_step": rline["ms_per_step"], "gflops": rline["value"],
                "achieved_GBs": rline["roofline"]["achieved"], "frac": rline["roofline"]["frac"],
                "gather_GBs": rline["roofline"]["gather_GBs"], "nnz": rline["config"]["nnz_per_gpu"],
                "generation_s": rline["config"]["generation_s"], "launch": rline["config"]["launch"],
                "verified_vs_oracle": rline["verified_vs_oracle"], "cpu_baseline": rline["cpu_baseline"],
                "note": "run_rmat() with world = 1: what the N > 1 SCALE lines call `one_gpu_reference`"}
            torch.cuda.empty_cache()

        # ---- boundary #1 in the record: the `spmm_test` driver (reference CLI and protocol: 200 timed launches per width,
        #      N in {128, 256, 512}, vendor column = rocSPARSE where the reference has cuSPARSE, spmm_test.cu:714-762) on the
        #      headline graph written as a MatrixMarket file; default method (2, what the reference times) and AUTO through a plan
        try:
            import re
            import subprocess
            import tempfile

            drv = os.path.join(ROOT, "gespmm_amd", "lib", "spmm_test")
            if os.path.exists(drv):
                with tempfile.TemporaryDirectory() as td:
                    mtx = os.path.join(td, graph + ".mtx")
                    graphs.write_mtx(mtx, g["rowptr"], g["colind"])
                    rows_ = {}
                    for label, more in (("method2_reference_default", []), ("auto_plan", ["--method", "-1", "--plan"])):
                        r = subprocess.run([drv, mtx, str(local_rank), "--out", os.path.join(td, "csv.out"), "--seed", "1"] + more,
                                           capture_output=True, text=True, timeout=600)
                        rows_[label] = {
                            "N%s" % m.group(1): {"ms_per_iter": float(m.group(2)), "gflops": float(m.group(3)),
                                                 "rocsparse_gflops": float(m.group(4))}
                            for m in re.finditer(r"N=(\d+) method=-?\d+[^:]*: ([0-9.]+) ms/iter, ([0-9.]+) GFLOP/s \(rocsparse ([0-9.]+) GFLOP/s\)",
                                                 r.stdout)}
                        rows_[label]["exit_status"] = r.returncode
                    rows_["note"] = ("A == 1 as the reference's driver sets it (spmm_test.cu:574), B = rand()%100-50 with seed 1, host-side "
                                     "load + upload outside the timed loops, 200 launches per figure")
                    extra["driver_spmm_test"] = rows_
        except Exception as ex:  # noqa: BLE001
            extra["driver_spmm_test"] = {"skipped": "%s: %s" % (type(ex).__name__, str(ex)[:200])}

        # ---- the reference's own kernels on this MI355X (oracle/_ref/libref_kernels.so: spmm_test.cu compiled by hipcc
        #      as it is — a baseline leg, never the product): spmmWrapper(method 2, tile_row 8), what the reference times
        #      (spmm_test.cu:756), on the headline operands — A == 1 as its driver sets it, and with the bench's values
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import ref_py

            if ref_py.kernels_available() and K * N < (1 << 31):  # the reference pre-multiplies column indices in int32
                torch.cuda.empty_cache()
                Br = make_B(K, N)
                Cr = torch.empty((M, N), dtype=torch.float32, device=dev)
                ones = torch.ones(nnz, dtype=torch.float32, device=dev)
                refk = {}
                for label, vv in (("A=1", ones), ("valued", val)):
                    def rstep():
                        ref_py.spmm_wrapper(2, 8, g["rowptr"], g["colind"], vv, Br, out=Cr, sync=False)
                    for _ in range(5):
                        rstep()
                    medr = statistics.median(kernel_times_us(rstep, MIN_KERNEL_SAMPLES))
                    refk[label] = {"kernel_us": medr, "gflops": 2.0 * nnz * N / medr / 1e3,
                                   "frac": abytes / medr / 1e3 / HBM_PEAK_GBS}
                mine = spmm.csr_spmm(g["rowptr"], g["colind"], val, Br)
                refk["product_bits_equal_reference_kernel"] = bool(torch.equal(mine.view(torch.int32), Cr.view(torch.int32)))
                refk["what"] = ("spmm_test2<float> (CRC + CWM CF2, block (32, 8)) from /root/reference/spmm_test.cu:161-236, "
                                "hipcc --offload-arch=gfx950 -O3, launched through the reference's spmmWrapper on the null stream")
                extra["reference_kernels_on_this_gpu_N%d" % N] = refk
                reference_kernel = {"what": "reference spmm_test2 (hipcc, gfx950) on the same operands",
                                    "kernel_us": refk["valued"]["kernel_us"], "gflops": refk["valued"]["gflops"],
                                    "product_bits_equal": refk["product_bits_equal_reference_kernel"]}
                del Br, Cr, ones, mine
        except Exception as ex:  # noqa: BLE001 - a baseline leg must never take the bench line down
            extra["reference_kernels_on_this_gpu_N%d" % N] = {"skipped": "%s: %s" % (type(ex).__name__, str(ex)[:200])}

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baselines(graphs, torch, g, val, N, graph, quick=args.no_extra)

    if rank == 0:
        out = {
            "metric": "SpMM GFLOP/s (= 2*nnz*N/t), CSR x dense fp32, N=%d" % N,
            "value": value,
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": ("%s (M=K=%d, nnz=%d per GPU, symmetric, seed 42+rank, locality %.2f) x N=%d, valued CSR, "
                             "variant %d" % (graph, M, nnz, args.locality, N, args.variant)),
                "rows_per_gpu": M,
                "nnz_per_gpu": nnz,
                "ncols": N,
                "launch": ("gespmm_plan_spmm_f32 (analysis stage once, outside the timed region: %s)" % head.get("plan"))
                          if not args.no_plan else "gespmm_csr_spmm_f32 (no plan)",
                "partition": "independent replicas, one graph per rank (the row-partitioned experiment is --graph rmat)"
                             if world > 1 else "single GPU",
                "stand_in": ("seeded stand-in for SNAP com-Amazon (no network): planted communities, clustering 0.408 (SNAP: 0.397), "
                             "ids shuffled; the structureless one (rounds 1-2's headline) is series['com-amazon-like']"
                             if graph == "com-amazon-sbm" else
                             "seeded structureless stand-in for SNAP com-Amazon (clustering 4e-5); the planted-community one is "
                             "series['com-amazon-sbm']") if graph.startswith("com-amazon") else graph,
            },
            "roofline": {
                "bound": "hbm",
                "achieved": head["achieved_GBs"],
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": head["frac"],
                "traffic": traffic,
                "traffic_source": traffic_src,
                "l2_hit_rate": l2_hit,
                "algorithmic_bytes_per_launch": abytes,
                "kernel_us": head["kernel_us"],
                "launches": head.get("launches"),
                "kernel_us_stat": "average over the %d launches of the timed region, one HIP event pair around the region" % args.steps,
                "kernel_us_median_of_pairs": head["kernel_us_median_of_pairs"],
                "kernel_us_mean": head.get("kernel_us_mean"),
                "kernel_us_min": head.get("kernel_us_min"),
                "roof_gflops": roof_gflops(M, K, N, nnz, True),
                "gflops_kernel": head["gflops"],
                # diagnostic: B-row gathers without reuse, 4*nnz*N bytes, and their rate
                "gather_bytes_per_launch": 4 * nnz * N,
                "gather_GBs": 4.0 * nnz * N / head["kernel_us"] / 1e3,
            },
            "plan_ms": head.get("plan_ms"),
            "plan_ms_first_creation": head.get("plan_ms_first_creation"),
            # what a caller that runs the reference's protocol (200 launches, spmm_test.cu:714) gets with the analysis
            # stage INSIDE the time; the plain entry point (no analysis) is extra.plain_call_*: compare the two
            "value_incl_plan_over_200_launches": head.get("gflops_incl_plan_over_200_launches"),
            # ... and priced with the FIRST creation of this process (after gespmm_init, whose time is `init_ms`: start-up, like loading
            # the library; a process that skips gespmm_init pays ~32 ms more for its first plan — profiles/r06/plan_cold.log)
            "value_incl_first_plan_over_200_launches": head.get("gflops_incl_first_plan_over_200_launches"),
            "init_ms": init_ms,
            "stateless_auto_plan": stateless,
            "cpu_baseline": cpu,
            "verified_vs_oracle": verified,
            "series": {k: {kk: _r(vv) for kk, vv in v.items()} for k, v in series.items()} or None,
            "widths": {k: {kk: _r(vv) for kk, vv in v.items()} for k, v in widths.items()} or None,
            "reference_kernel": {kk: _r(vv) for kk, vv in reference_kernel.items()} if reference_kernel else None,
            "other_configs": other_configs(extra) or None,
            "extra": extra,
        }
        out["roofline"].update(ceiling_for(g, N, head["frac"]))
        out["roofline"]["copy_rate_GBs"] = copy_rate
        out["config"]["kernel"] = (head.get("plan") or "").split("|")[-1].strip()[:120] if head.get("plan") else "plain call"
        emit(out)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def other_configs(extra):
    """BASELINE configs 1-5 beside the headline, one number each (kernel time through the library's own choice, frac of the
    HBM roofline); everything else about them is in the side file."""
    out = {}

    def put(name, e):
        if isinstance(e, dict) and "kernel_us" in e:
            out[name] = {"ms": _r(e["kernel_us"] / 1e3, 2), "frac": _r(e.get("frac"), 2)}
            if e.get("ceiling_frac") is not None:  # stand-ins with planted structure: where that structure caps frac, and how close
                out[name]["ceil"] = _r(e["ceiling_frac"], 2)
                out[name]["of_ceil"] = _r(e["achieved_over_ceiling"], 2)

    for k, e in extra.items():
        if k.startswith(("reddit-", "cit-hepth", "pubmed", "rmat-", "powerlaw-")):
            put(k.replace("_valued", "").replace("_unweighted", ""), e)
        if k.endswith("_sweep_valued"):
            rows_ = {w: r for w, r in e.items() if isinstance(r, dict) and "plan" in r and isinstance(r["plan"], dict)}
            out[k.replace("_sweep_valued", "_plan_ms")] = {w: _r(r["plan"]["kernel_us"] / 1e3, 2) for w, r in rows_.items()}
            if any("ceiling_frac" in r["plan"] for r in rows_.values()):  # frac / ceiling_frac / achieved_over_ceiling per width
                out[k.replace("_sweep_valued", "_frac_ceil_ofceil")] = {
                    w: [_r(r["plan"]["frac"], 2), _r(r["plan"]["ceiling_frac"], 2), _r(r["plan"]["achieved_over_ceiling"], 2)]
                    for w, r in rows_.items() if "ceiling_frac" in r["plan"]}
    return out


def csrc_fingerprint():
    """sha256 over the kernel / launcher sources (what decides the traffic of a launch), first 16 hex digits."""
    import glob
    import hashlib

    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "gespmm_amd", "csrc", "*"))):
        if os.path.isfile(f) and not f.endswith((".o", ".so")):
            h.update(os.path.basename(f).encode())
            with open(f, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


def cpu_baselines(graphs, torch, g, val, N, graph, quick=False):
    """The reference's CPU loop (oracle restatement, i->k->ptr, fp32 accumulator) on this box's host cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np

    import oracle_py

    try:  # the reference's OWN golden loop (spmm_test.cu:596-604 compiled from the checkout: oracle/_ref/libref_host.so)
        import ref_py

        have_ref = ref_py.available()
    except Exception:  # noqa: BLE001
        ref_py, have_ref = None, False
    kind = "reference" if have_ref else "port"

    def time_pass(rph, cih, vh, Bh, mode, reps):
        """mode 'golden' = the single-threaded loop: the reference's lines when oracle/_ref is there, else the oracle's restatement
        (pinned to them bit for bit, tests/test_ref_pin.py); 'omp' = the oracle's OpenMP form of the same loop body."""
        best = None
        ones = np.ones(cih.shape[0], dtype=np.float32) if (vh is None and have_ref and mode == "golden") else None
        for _ in range(reps):
            t0 = time.perf_counter()
            if have_ref and mode == "golden":
                ref_py.golden(rph, cih, vh if vh is not None else ones, Bh)
            else:
                oracle_py.spmm(rph, cih, vh, Bh, mode)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best

    def full(gx, vx, n, reps=3):
        rph, cih = gx["rowptr"].cpu().numpy(), gx["colind"].cpu().numpy()
        vh = vx.cpu().numpy() if vx is not None else None
        Bh = np.ascontiguousarray(((np.random.RandomState(1).randint(0, 100, (gx["K"], n)) - 50) / 100).astype(np.float32))
        one = time_pass(rph, cih, vh, Bh, "golden", reps)
        oracle_py.spmm(rph, cih, vh, Bh, "omp")  # warm pass: thread pool, page faults
        allc = time_pass(rph, cih, vh, Bh, "omp", 3)
        fl = 2.0 * gx["nnz"] * n
        return {"value": fl / one / 1e9, "cores": 1, "all_cores": {"value": fl / allc / 1e9, "cores": oracle_py.num_threads()},
                "gflop_per_pass": fl / 1e9}

    def sampled(gx, n, frac=0.01, seed=0):
        """>= 1 % of the rows (contiguous blocks of 64, every B row they touch), full width."""
        rph = gx["rowptr"].cpu().numpy()
        M = gx["M"]
        rng = np.random.RandomState(seed)
        nblk = max(1, int(M * frac) // 64 + 1)
        starts = np.sort(rng.choice(max(M // 64, 1), min(nblk, max(M // 64, 1)), replace=False)) * 64
        rows = np.unique(np.concatenate([np.arange(s, min(s + 64, M)) for s in starts]))
        sub_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
        sub_ptr[1:] = np.cumsum(rph[rows + 1] - rph[rows])
        sel = torch.from_numpy(np.concatenate([np.arange(rph[r], rph[r + 1]) for r in rows]).astype(np.int64)).to(gx["colind"].device)
        cih = gx["colind"][sel].cpu().numpy()
        cols_u, inv = np.unique(cih, return_inverse=True)
        Bh = np.ascontiguousarray(((np.random.RandomState(2).randint(0, 100, (len(cols_u), n)) - 50) / 100).astype(np.float32))
        one = time_pass(sub_ptr, inv.astype(np.int32), None, Bh, "golden", 2)
        oracle_py.spmm(sub_ptr, inv.astype(np.int32), None, Bh, "omp")
        allc = time_pass(sub_ptr, inv.astype(np.int32), None, Bh, "omp", 3)
        fl = 2.0 * int(sub_ptr[-1]) * n
        return {"value": fl / one / 1e9, "cores": 1, "all_cores": {"value": fl / allc / 1e9, "cores": oracle_py.num_threads()},
                "sample": "%d rows (%.1f %% of M, blocks of 64), %.2f GFLOP; B restricted to the %d rows they touch" %
                          (len(rows), 100.0 * len(rows) / M, fl / 1e9, len(cols_u))}

    head = full(g, val, N)
    cpu = {
        "value": head["value"],
        "unit": "GFLOP/s",
        "cores": 1,
        "kind": kind,
        "what": ("the reference's own CPU loop, spmm_test.cu:596-604 compiled from the checkout by oracle/make_ref.sh (g++ -O3)" if have_ref
                 else "oracle restatement of spmm_test.cu:596-604 (gcc -O3), pinned to the reference's lines bit for bit"),
        "sample": "full %s x N=%d pass (%.2f GFLOP), best of 3, reference loop order i->k->ptr" % (graph, N, head["gflop_per_pass"]),
        "all_cores": dict(head["all_cores"], note="same loop body, OpenMP over rows, best of 3 after one warm pass"),
    }
    if not quick:
        dev = g["rowptr"].device
        others = {}
        g1 = graphs.synthetic_graph("cit-hepth-like", seed=42, device="cpu")
        others["C1 cit-hepth-like x N=32 (full, unweighted)"] = full(g1, None, 32)
        g4 = graphs.synthetic_graph("pubmed-selfloop-like", seed=42, device="cpu")
        others["C4 pubmed+selfloops-like x N=128 (full, unweighted)"] = full(g4, None, 128)
        torch.cuda.empty_cache()
        g2 = graphs.synthetic_graph("reddit-like", seed=42, device=dev)
        others["C2b reddit-like x N=128 (row sample)"] = sampled(g2, 128)
        del g2
        torch.cuda.empty_cache()
        g3 = graphs.synthetic_graph("products-like", seed=42, device=dev)
        others["C3 products-like x N=128 (row sample)"] = sampled(g3, 128)
        del g3
        cpu["others"] = others
    return cpu


def rmat_cpu_baseline(torch, g, N):
    """The reference's CPU loop on a row sample of the RMAT shard (contiguous blocks of 64 rows, ~2 * 10^6 entries, every B
    row they touch): 1 core and all cores, as for the reddit- and products-shaped graphs."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np

    import oracle_py

    M, nnz = g["M"], g["nnz"]
    rph = g["rowptr"].cpu().numpy()
    target = 2_000_000
    nblk = max(1, int(target / max(nnz / max(M, 1), 1e-9)) // 64)
    rng = np.random.RandomState(0)
    starts = np.sort(rng.choice(max(M // 64, 1), min(nblk, max(M // 64, 1)), replace=False)) * 64
    rows = np.unique(np.concatenate([np.arange(s0, min(s0 + 64, M)) for s0 in starts]))
    sub_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    sub_ptr[1:] = np.cumsum(rph[rows + 1] - rph[rows])
    sel = torch.from_numpy(np.concatenate([np.arange(rph[r], rph[r + 1]) for r in rows]).astype(np.int64)).to(g["colind"].device)
    cih = g["colind"][sel].cpu().numpy()
    cols_u, inv = np.unique(cih, return_inverse=True)
    Bh = np.ascontiguousarray(((np.random.RandomState(2).randint(0, 100, (len(cols_u), N)) - 50) / 100).astype(np.float32))
    inv = inv.astype(np.int32)

    try:
        import ref_py

        have_ref = ref_py.available()
    except Exception:  # noqa: BLE001
        ref_py, have_ref = None, False
    ones = np.ones(int(sub_ptr[-1]), dtype=np.float32)

    def best(mode, reps):
        t = None
        for _ in range(reps):
            t0 = time.perf_counter()
            if have_ref and mode == "golden":
                ref_py.golden(sub_ptr, inv, ones, Bh)  # the reference's own loop (oracle/_ref)
            else:
                oracle_py.spmm(sub_ptr, inv, None, Bh, mode)
            dt = time.perf_counter() - t0
            t = dt if t is None else min(t, dt)
        return t

    one = best("golden", 2)
    oracle_py.spmm(sub_ptr, inv, None, Bh, "omp")
    allc = best("omp", 3)
    fl = 2.0 * int(sub_ptr[-1]) * N
    return {"value": fl / one / 1e9, "unit": "GFLOP/s", "cores": 1, "kind": "reference" if have_ref else "port",
            "all_cores": {"value": fl / allc / 1e9, "cores": oracle_py.num_threads()},
            "sample": "%d rows (%.3f %% of M, blocks of 64), %.2f GFLOP; B restricted to the %d rows they touch" %
                      (len(rows), 100.0 * len(rows) / M, fl / 1e9, len(cols_u))}


def run_rmat(args, env, N, with_cpu_baseline=False, full=True):
    """ONE RMAT graph, nnz-balanced contiguous row shards, B replicated by all-gather: the north_star experiment.
    `env` (BenchEnv) carries the device, the process group and the product — see its docstring. `full` = False (a plain
    `bench.py` run) times the kernel-only loop and nothing beside it: no per-launch event pairs (their launches run untimed; the
    roofline is priced with the timed region, as the one-GPU line is), no sampled-row check, no end-to-end panel pipeline."""
    from gespmm_amd import dist as gdist
    from gespmm_amd import graphs

    torch, dist, dev, world, rank, use_dist = env.torch, env.dist, env.dev, env.world, env.rank, env.use_dist
    scale = args.rmat_scale or 26
    t0 = time.perf_counter()
    g = graphs.rmat_shard(scale, args.edge_factor, rank, world, seed=42, device=dev)
    env.device_sync()
    gen_s = time.perf_counter() - t0
    M, K, nnz = g["M"], g["K"], g["nnz"]
    rowptr, colind = g["rowptr"], g["colind"]
    val = torch.rand(nnz, generator=env.generator(7 + rank), device=dev) - 0.5
    if use_dist:
        tn = torch.tensor([nnz], dtype=torch.int64, device=dev)
        dist.all_reduce(tn)
        nnz_total = int(tn.item())
    else:
        nnz_total = nnz

    # ---- every rank owns K/world rows of B (its own seed); one all-gather replicates them
    k0, k1 = (K * rank) // world, (K * (rank + 1)) // world
    B_shard = env.make_B(k1 - k0, N, seed=5000 + rank)
    counts = [(K * (r + 1)) // world - (K * r) // world for r in range(world)]
    env.sync_all()
    t0 = time.perf_counter()
    B = gdist.exchange_dense(B_shard, counts) if use_dist else B_shard
    env.sync_all()
    exchange_ms = (time.perf_counter() - t0) * 1e3 if use_dist else 0.0

    # ---- kernel only: B resident (the BENCH line's convention)
    C = torch.empty((M, N), dtype=torch.float32, device=dev)
    plan = env.make_plan(rowptr, colind, K, N, val)

    def step():
        env.product(rowptr, colind, val, B, C, plan)

    for _ in range(max(args.warmup, 1)):
        step()
    if full:
        us = env.kernel_times_us(step, max(args.steps, 5))
    else:  # the same launches untimed: both modes start the timed region from the same device state (see main())
        us = None
        for _ in range(max(args.steps, 5)):
            step()
    wall = env.timed_region(step, args.steps, 0)
    if getattr(args, "dump_outputs", None) and rank == 0:
        dump_outputs(args.dump_outputs, C)
    value = 2.0 * nnz_total * N * args.steps / wall / 1e9
    med = statistics.median(us) if full else env.region_event_us
    verified = env.verify(rowptr, colind, val, B, C, nrows=256, tolerant=True) if rank == 0 and full else None
    if env.on_local_product is not None:  # (the CPU suite gathers the shards' rows and compares them with the unsharded product)
        env.on_local_product(g, val, B, C)
    abytes = algorithmic_bytes(M, K, N, nnz, True)
    srows = torch.randperm(M, device=dev)[:4096]
    C_sample = C[srows].clone()
    del C

    # ---- end to end: column panels, exchange of panel p+1 overlapped with the product of panel p
    e2e = None
    pc = max(4, min(args.panel_cols, N))
    need = 4.0 * ((k1 - k0) * N + 2 * K * pc + M * N) * 1.02  # panel copies of the shard, two panel buffers, C panels
    if full and use_dist and need > env.free_bytes() + 4.0 * K * N:
        e2e = {"skipped": "panel buffers exceed free HBM at this scale on %d GPU(s)" % world}
    elif full and use_dist:
        def end_to_end():
            nonlocal B, plan
            del B, plan
            env.empty_cache()
            panels = [(c0, min(c0 + pc, N)) for c0 in range(0, N, pc)]
            pipe = gdist.PanelPipeline(rowptr, colind, val, K, counts, [c1 - c0 for c0, c1 in panels], dev, variant=env.variant,
                                       product=env.injected_product)
            shard_panels = [B_shard[:, c0:c1].contiguous() for c0, c1 in panels]
            pipe.run(shard_panels)  # warm
            env.sync_all()
            reps = max(1, min(args.steps, 3))
            t0 = time.perf_counter()
            for _ in range(reps):
                Cp = pipe.run(shard_panels)
            env.sync_all()
            e2e_s = env.max_over_ranks((time.perf_counter() - t0) / reps)
            # panel results against the resident-B product on sampled rows (hub rows take the long-row pass, whose chunk sums
            # are grouped by the lane geometry of the width: those rows agree to rounding, all others bit for bit)
            same, worst = 0, 0.0
            for (c0, c1), cp in zip(panels, Cp):
                a_, b_ = cp[srows], C_sample[:, c0:c1]
                same += int((a_.view(torch.int32) == b_.contiguous().view(torch.int32)).all(dim=1).sum())
                worst = max(worst, float(((a_ - b_).abs() / (b_.abs() + 1e-3)).max()))
            return {"ms_per_product": e2e_s * 1e3, "gflops": 2.0 * nnz_total * N / e2e_s / 1e9, "panel_cols": pc,
                   "panels": len(panels), "sampled_rows_bit_equal_resident_product": "%d of %d" % (same, len(panels) * int(srows.numel())),
                   "max_rel_diff_vs_resident_product": worst,
                   "note": "all-gather of panel p+1 on a second stream while panel p is multiplied; exchange inside the timed region"}

        try:
            e2e = end_to_end()
        except Exception as ex:  # noqa: BLE001 - the kernel-only line above must still be reported
            e2e = {"failed": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
            env.empty_cache()

    L = 64
    kernel_s = wall / args.steps
    cpu = None
    if with_cpu_baseline and rank == 0 and world == 1:
        cpu = rmat_cpu_baseline(torch, g, N)
    return {
        "metric": "SpMM GFLOP/s (= 2*nnz*N/t), CSR x dense fp32, N=%d" % N,
        "value": value,
        "unit": "GFLOP/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": kernel_s * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": ("RMAT scale %d edge-factor %d (a,b,c,d = .57,.19,.19,.05), %d global nnz, nnz-balanced row shards "
                         "x N=%d, valued CSR, variant %d" % (scale, args.edge_factor, nnz_total, N, args.variant)),
            "rows_per_gpu": M,
            "nnz_per_gpu": nnz,
            "ncols": N,
            "partition": "1-D rows (nnz-balanced shards of one graph), B owned as K/world row shards, replicated by RCCL all-gather"
                         if world > 1 else "single GPU",
            "launch": "gespmm_plan_spmm_f32 (storage order: the longest row decides the long-row pass)",
            "generation_s": gen_s,
        },
        "roofline": {
            "bound": "hbm", "achieved": abytes / med / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": abytes / med / 1e3 / HBM_PEAK_GBS,
            "traffic": None, "algorithmic_bytes_per_launch": abytes, "kernel_us": med,
            "kernel_us_stat": ("median of %d event pairs around %d launch(es) each (rank 0)" % (len(us), env.launches_per_event_pair) if full
                               else "average over the %d launches of the timed region, one HIP event pair around the region (rank 0)" % args.steps),
            "gather_bytes_per_launch": 4 * nnz * N, "gather_GBs": 4.0 * nnz * N / med / 1e3,
        },
        "exchange": {
            "replicate_B_ms": exchange_ms,
            "bytes_received_per_gpu": 4 * (K - (k1 - k0)) * N,
            "kernel_only_gflops": value,
            "end_to_end": e2e,
            "amortised_over_L": {"L": L, "gflops": 2.0 * nnz_total * N * L / (exchange_ms / 1e3 + L * kernel_s) / 1e9,
                                 "note": "one replication of B reused by L products (layers x epochs of a static feature matrix)"},
        },
        "one_gpu_reference": ("extra['rmat-%d_N256_valued'] of the N = 1 line of the same driver run: this graph, this code "
                              "path (run_rmat with one rank)" % scale) if world > 1 else "this line",
        "cpu_baseline": cpu,
        "verified_vs_oracle": verified,
    }


if __name__ == "__main__":
    main()
