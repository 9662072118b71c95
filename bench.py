#!/usr/bin/env python3
"""bench.py -- graphs/sec of the MaskEmbdMultiMPN hot path on MI355X (BASELINE.json's metric).

One "step" = one pass of the hot path over one batch already resident in HBM: forward, MSELoss, backward,
(DP: one flat-buffer gradient all-reduce) and the AdamW update -- the per-batch body of the reference's
train_epoch (utils/training.py:55-77) minus the host->device copy and the loss.item() sync.  Default workload:
case118v2 (118 buses / 186 branches, synthetic topology per SURVEY.md 8d), batch 128 per GPU, standard.json
(H=129, L=4, K=3, dropout 0.2), fp32, weak scaling across ranks.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus N ...            (no torchrun environment: starts its own N ranks, one per GPU, on a free port)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --mode infer --batch 1  (per-sample latency: the one timing the reference itself takes,
                                             perfomance_evaluator.py:61-74)

Rank 0 prints ONE JSON line.  A plain run measures only the headline: set-up, warm-up, the K timed steps, the line.  The timed
region starts from the training state the three eager warm-up steps left (restored after the clock ramp and the W warm-up
steps), so the same arguments give the same last step on every run and every build: `--dump-outputs DIR` writes what that
step computed (DIR/<name>.npy, float32).  `--full` adds everything else the line can carry:
  roofline     : dominant kernel class, algorithmic bytes|flops per launch / HIP-event launch duration
  cpu_baseline : the CPU oracle (oracle/ref_cpu.py, kind "port") timed on this box's host cores, bounded sample
  kernels      : per-kernel-class table behind `roofline` (count per step, avg us, achieved, fraction of peak)
  median / min step time, eager / new-topology / reference-loop / world-1-RCCL step times, the isolated scatter-add, and
  short runs of BASELINE.json's other single-GPU configurations (`other_configs`)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # B/s, MI355X spec (MI355X_MICROARCH.md; ~6.3e12 achievable)
MFMA_F32_PEAK = 157.3e12  # FLOP/s, v_mfma_f32_32x32x2_f32 / 16x16x4 (no TF32/xf32 on gfx950)
CONFIGS = {"standard": (129, 4, 3), "wide": (129, 6, 6), "small": (64, 2, 3), "large": (512, 5, 3)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clock-ramp-ms", type=float, default=250.0,
                    help="untimed replays BEFORE the W warm-up steps until this much wall time has passed: a fresh GPU needs "
                         "~0.1-0.2 s of load before its clocks and power state settle (with --warmup 5 --steps 20 the timed "
                         "region is 13 ms and read 3 %% slow without it); 0 disables")
    ap.add_argument("--case", default="118v2")
    ap.add_argument("--batch", type=int, default=128, help="graphs per GPU")
    ap.add_argument("--config", default="standard", choices=sorted(CONFIGS))
    ap.add_argument("--mode", default="train", choices=["train", "infer"])
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--dp-mode", default=None, choices=["graph", "split", "eager"],
                    help="launch form of the (data-parallel) training step: one hipGraph incl. the RCCL all-reduce (default), "
                         "graph / eager all-reduce / graph, or eager launches; ranks always agree on it (dp.GraphedStep)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--hub-frac", type=float, default=0.0)
    ap.add_argument("--no-dp-overhead", action="store_true",
                    help="skip the world-size-1 RCCL step (graph-captured all-reduce) that prices the collective at N = 1")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)   # a counter pass of live_traffic(): timing loops only
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="skip the two rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE) behind roofline.traffic")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short runs of BASELINE.json's other single-GPU configurations (reported under `other_configs`)")
    ap.add_argument("--loss", default="mse", choices=["mse", "masked_l2"],
                    help="mse = BASELINE.json's metric (train.py:103); masked_l2 = the reference's default --train_loss_fn")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: median / min step time, the per-kernel pass (--profile-steps) and roofline, live "
                         "traffic, the eager and reference-loop step times, the isolated scatter-add, the CPU baseline and the "
                         "other configurations (the --no-* switches above thin this set out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32): `output` (the "
                         "model's prediction), and in training `loss` and `params` (the flat parameter buffer after AdamW)")
    return ap.parse_args()


DUMP_BUDGET = 64 << 20      # bytes, all arrays of --dump-outputs together


def dump_outputs(outdir, arrays):
    """Write {name: device tensor} as outdir/<name>.npy in float32.  Arrays that together exceed DUMP_BUDGET are replaced by a
    fixed sample of their flattened entries (numpy default_rng(0), indices sorted) of each array's share of the budget."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    share = DUMP_BUDGET // (4 * max(len(host), 1))
    for name, a in host.items():
        if total > DUMP_BUDGET and a.size > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))]
        np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def alg_bytes(n, e, h, fe, K=3, train=True):
    """Algorithmic bytes per launch of the gather/segment-sum kernel classes (4-byte elements and indices; logical
    inputs once, one gathered row per directed edge, output once -- the convention of SURVEY.md 8d)."""
    return {
        "hop_norm": 4.0 * (e * h + e + n * h + (n + 1)),                          # B_sa(H)
        "scatter_add": 4.0 * (e * h + e + n * h + (n + 1)),
        # K hops in one launch, rows LDS-resident between hops: the kernel's OWN minimum traffic -- read x once, write the K hop
        # outputs, indices once -- is the roofline denominator (K x B_sa(H), what K unfused hops would move, is reported beside
        # it as `equiv_unfused`: bytes this kernel by design never touches)
        "fused_hops_fwd": 4.0 * (n * h + K * n * h + e + (n + 1)),
        "fused_hops_bwd": 4.0 * (n * h + K * n * h + e + (n + 1)),
        # the LDS-resident edge stage of big inference batches of small graphs: its OWN minimum traffic -- P, Q read once, S written,
        # attributes and indices once (the per-edge gathers of the generic kernel never leave LDS here)
        "edge_rows_fwd": 4.0 * (3 * n * h + e * fe + 2 * e + (n + 1)),
        # training: the forward walk also saves one ReLU-mask byte per (edge, float4 chunk) ...
        "edge_fwd": 4.0 * (n * h + e * h + e * fe + e + (n + 1) + n * h) + (e * ((h + 3) // 4) if train else 0),
        # ... and the backward walks (one launch: the by-destination half -> dP, dWe; the by-source half -> dQ) read the masks
        # instead of recomputing: dS once + its row gathered once per edge, the masks twice, indices, two outputs
        "edge_bwd": 4.0 * (n * h + e * fe + e + (n + 1) + n * h) + 4.0 * (e * h + 3 * e + (n + 1) + n * h) + 2.0 * e * ((h + 3) // 4),
    }


def b_fwd(n, e, h, L, K, f0=4, fo=4, fe=2):
    """B_fwd = B_EA(F0->H) + (L-2) B_EA(H->H) + B_EA(H->Fo) + (L-1) B_TAG + B_mask."""
    b_ea = lambda fi, fo_: 4.0 * (n * fi + e * fi + e * fe + e + (n + 1) + n * fo_)
    b_tag = K * 4.0 * (e * h + e + n * h + (n + 1)) + 4.0 * n * (h + h)
    return b_ea(f0, h) + (L - 2) * b_ea(h, h) + b_ea(h, fo) + (L - 1) * b_tag + 48.0 * n


def cpu_baseline(args, cfg, data_cpu, seconds):
    """The CPU oracle (pure-torch restatement of the reference dataflow) timed on this box's host cores.  torch's
    intra-op pool over-subscribes badly on many-core hosts (256 threads: ~70 s/step on this workload), so the thread
    count is the best of a short sweep -- the most favourable setting for the CPU side; `cores` reports it."""
    from oracle import ref_cpu
    h, L, K = cfg
    ncpu = os.cpu_count() or 1
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, h, L, K, 0.2)
    B = args.batch
    if args.mode == "train":
        ref.train()
        opt = torch.optim.AdamW(ref.parameters(), lr=1e-3)
        step = lambda: ref_cpu.train_step(ref, data_cpu, opt)
    else:
        ref.eval()

        def step():
            with torch.no_grad():
                ref(data_cpu)
    best_t, best_n = None, 1
    for nt in sorted({n for n in (4, 8, 16, 32, 64) if n <= ncpu} | ({ncpu} if ncpu <= 64 else set())):
        torch.set_num_threads(nt)
        step()                                        # warm-up at this thread count
        t0 = time.perf_counter()
        step()
        dt = time.perf_counter() - t0
        if best_t is None or dt < best_t:
            best_t, best_n = dt, nt
        if dt > 30:                                   # keep the default run within minutes
            break
    torch.set_num_threads(best_n)
    t0, n = time.perf_counter(), 0
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or n >= 50:
            break
    return {"value": round(B * n / dt, 2), "unit": "graphs/s", "cores": best_n, "kind": "port",
            "sample": f"{n} {args.mode} steps of the same workload (case{args.case} batch={B}, {args.config}) on the "
                      f"pure-torch CPU restatement of the reference dataflow, {dt:.1f} s, torch threads={best_n} "
                      f"(best of a 4..64 sweep; host has {ncpu} logical cores)",
            "host_logical_cores": ncpu, "ms_per_step": round(1e3 * dt / n, 2)}


KERNEL_OF_CLASS = {"gemm_nt": "gemm_nt_kernel", "gemm_tn": "gemm_tn_kernel", "hop_norm": "hop_kernel<true", "edge_fwd": "edge_fwd_", "edge_rows_fwd": "edge_rows_fwd_kernel",
                   "edge_bwd": "edge_bwd_", "fused_hops_fwd": "_hops_kernel(", "fused_hops_bwd": "_hops_kernel(",
                   "ea_seg_fwd": "ea_seg_fwd_kernel", "ea_seg_bwd": "ea_seg_bwd_kernel",
                   "seg_lin_hops_fwd": "seg_lin_hops_kernel<1>", "seg_lin_hops_bwd": "seg_lin_hops_kernel<2>", "front_fwd": "front_fwd", "front_bwd": "front_bwd"}


def under_profiler() -> bool:
    env = os.environ
    return any(k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_")) for k in env) or "rocprofiler" in env.get("LD_PRELOAD", "")


def live_traffic(args, klass):
    """HBM-side bytes per launch of kernel class `klass`, measured NOW: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE: they
    do not fit one pass) over a short eager run of this very workload in a child process, corrected as MI355X_MICROARCH.md
    prescribes for gfx950 (FETCH_SIZE counts a 128-byte request of a wide coalesced read as 64 bytes: x 2; counter unit KiB).
    The counters sit on the fabric side of L2 and include Infinity-Cache hits.  Returns (bytes, detail) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    if under_profiler():
        return None, "already running under a profiler"
    pat = KERNEL_OF_CLASS.get(klass)
    if pat is None:
        return None, f"no kernel-name pattern for class {klass}"
    child = [sys.executable, os.path.abspath(__file__), "--child", "--full", "--no-graph", "--steps", "2", "--warmup", "1", "--profile-steps", "0",
             "--clock-ramp-ms", "0",
             "--no-cpu-baseline", "--no-live-traffic", "--no-dp-overhead", "--case", str(args.case), "--batch", str(args.batch),
             "--config", args.config, "--mode", args.mode, "--hub-frac", str(args.hub_frac), "--loss", args.loss]
    tmp = tempfile.mkdtemp(prefix="pfn_traffic_", dir="/tmp")
    per = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            try:
                subprocess.run([exe, "--pmc", ctr, "--kernel-trace", "-f", "csv", "-d", d, "-o", "pmc", "--"] + child, cwd="/tmp",
                               env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                               timeout=240, check=True)
            except Exception as exc:              # noqa: BLE001
                return None, f"rocprofv3 --pmc {ctr} failed: {type(exc).__name__}"
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None, f"rocprofv3 --pmc {ctr} wrote no counter_collection.csv"
            n, tot = 0, 0.0
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") == ctr and pat in row.get("Kernel_Name", ""):
                        n += 1
                        tot += float(row["Counter_Value"])
            if n == 0:
                return None, f"no launch of {pat} in the {ctr} pass"
            per[ctr] = (tot / n, n)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    f_kib, w_kib = per["FETCH_SIZE"][0], per["WRITE_SIZE"][0]
    return int((2.0 * f_kib + w_kib) * 1024), {"FETCH_SIZE_KiB_per_launch": round(f_kib, 1), "WRITE_SIZE_KiB_per_launch": round(w_kib, 1),
                                                "launches_counted": per["FETCH_SIZE"][1], "formula": "(2 x FETCH_SIZE + WRITE_SIZE) x 1024"}


def dp_overhead(fb, opt, model, dev, steps, base_ms):
    """What the gradient collective costs a replayed step: the SAME step captured once more with a world-size-1 RCCL process
    group alive and `ncclAllReduce(AVG)` of the flat gradient buffer inside the hipGraph (dp.GraphedStep), timed like the
    headline loop.  (One rank: the collective moves no data over xGMI -- this prices the node in the graph and RCCL's launch
    path; the N > 1 cost is in the driver's scaling runs.)"""
    import socket
    import torch.distributed as dist
    from poweflownet_amd import dp
    if dist.is_initialized():
        return {}
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    try:
        with dp.stdout_to_stderr():               # (RCCL's version banner must not land on the JSON line's stdout)
            # an explicit store of our own: under torchrun (TORCHELASTIC_USE_AGENT_STORE) a tcp:// init_method makes this process
            # a CLIENT of a store nobody serves at that port, and init_process_group waits for it for half an hour
            import datetime
            store = dist.TCPStore("127.0.0.1", port, 1, is_master=True, timeout=datetime.timedelta(seconds=60))
            dist.init_process_group(backend="nccl", store=store, rank=0, world_size=1, device_id=dev,
                                    timeout=datetime.timedelta(seconds=120))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):         # creates the communicator outside any capture
                fb()
                dp.allreduce_gradients(model)
                opt.step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
        opt.zero_grad(set_to_none=True)
        gs = dp.GraphedStep(fb, opt.step, model, allreduce=True).capture()
        for _ in range(5):
            gs.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            gs.replay()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        return {"dp_world1_rccl_ms_per_step": round(ms, 4), "dp_overhead_ms": round(ms - base_ms, 4), "dp_graph_mode": gs.mode}
    except Exception as exc:                      # noqa: BLE001
        return {"dp_overhead_error": f"{type(exc).__name__}: {exc}"[:300]}
    finally:
        try:
            torch.cuda.synchronize()
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:                         # noqa: BLE001
            pass


def device_identity(dev, local_rank) -> str:
    """What makes this rank's GPU distinguishable from every other rank's: PCI domain:bus:device + the UUID the driver reports."""
    pr = torch.cuda.get_device_properties(dev)
    pci = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0), getattr(pr, "pci_device_id", 0))
    return f"hip:{local_rank} pci {pci} uuid {getattr(pr, 'uuid', '?')} {pr.name} ({getattr(pr, 'gcnArchName', '?')})"[:160]


def rank_roster(dev, local_rank, own_ms, world, dist_on):
    """`ranks` of the JSON line: every rank's device identity and ITS OWN ms per step over the timed region (the headline takes
    the maximum), all-gathered over the process group -- a line with n_gpus = N carries N distinct devices or says so."""
    ident = device_identity(dev, local_rank)
    if not dist_on:
        return {"ranks": [{"rank": 0, "device": ident, "ms_per_step": round(own_ms, 4)}], "distinct_devices": 1}
    buf = torch.zeros(168, dtype=torch.uint8, device=dev)
    raw = ident.encode()[:160]
    buf[:len(raw)] = torch.tensor(list(raw), dtype=torch.uint8)
    buf[160:168] = torch.tensor([own_ms], dtype=torch.float64).view(torch.uint8)
    allb = [torch.zeros_like(buf) for _ in range(world)]
    torch.distributed.all_gather(allb, buf)
    ranks = []
    for r, b in enumerate(allb):
        b = b.cpu()
        ranks.append({"rank": r, "device": bytes(b[:160].tolist()).rstrip(b"\0").decode(errors="replace"),
                      "ms_per_step": round(float(b[160:168].view(torch.float64).item()), 4)})
    pci = {x["device"].split(" uuid ")[0].split("pci ")[-1] + "|" + x["device"].split(" uuid ")[-1].split(" ")[0] for x in ranks}
    return {"ranks": ranks, "distinct_devices": len(pci)}


OTHER_CONFIGS = {   # BASELINE.json configs[2] and configs[3] (configs[1] is the headline; configs[4] = configs[3] per rank under --gpus 8)
    "case118v2 inference batch=2048": ["--mode", "infer", "--batch", "2048", "--steps", "20", "--warmup", "5"],
    "case6470rte training batch=64": ["--case", "6470rte", "--batch", "64", "--steps", "6", "--warmup", "2"],
}


def other_configs():
    """The default invocation with --full also times BASELINE.json's other single-GPU configurations, briefly (a child process each: its own
    workspace, a few replayed steps, the per-kernel pass for the dominant kernel's roofline fraction; no CPU baseline, no counter
    passes), so that the record a driver keeps of `python bench.py` holds a number for every configuration -- not a headline."""
    import subprocess
    out = {}
    for name, extra in OTHER_CONFIGS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--full", "--no-cpu-baseline", "--no-live-traffic", "--no-dp-overhead",
               "--no-other-configs", "--profile-steps", "2"] + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            d = json.loads(line[-1])
            rf = d.get("roofline") or {}
            out[name] = {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"], "steps": d["steps"],
                         "launch": d["config"]["launch"], "step_mfma_frac": d.get("step_mfma_frac"), "step_hbm_frac": d.get("step_hbm_frac"),
                         "dominant_kernel": rf.get("kernel"), "dominant_frac": rf.get("frac"), "dominant_bound": rf.get("bound"),
                         "kernels_ms_per_step": {k: v["ms_per_step"] for k, v in sorted(d.get("kernels", {}).items(),
                                                                                         key=lambda kv: -kv[1]["ms_per_step"])[:6]},
                         "kernels_sum_ms_per_step": d.get("kernels_sum_ms_per_step"), "fractions_rejected": d.get("fractions_rejected")}
        except Exception as exc:                  # noqa: BLE001
            out[name] = {"error": f"{type(exc).__name__}: {exc}"[:200]}
    return out


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a torchrun environment: re-run this very command line under torch.distributed.run
    (one process per GPU, RCCL over xGMI, rendezvous on 127.0.0.1 at a free port).  Returns the launcher's exit code."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not os.environ.get("PFN_SINGLE_DEVICE"):
        print(f"bench.py: --gpus {args.gpus} but only {ndev} HIP device(s) are visible", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes needs it on this driver)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    try:   # the flat gradient views are produced on the capture stream on purpose
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    except Exception:
        pass
    args = parse()
    if os.environ.get("PFN_HANG_DUMP"):   # debugging aid: dump every thread's stack if the run is still alive after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["PFN_HANG_DUMP"]), exit=False)
    from poweflownet_amd import _lib as L
    from poweflownet_amd import dp
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.synth import CASES, make_batch

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))      # no torchrun environment: start the N ranks ourselves (rank 0 prints the JSON line)
    rank, local_rank, world = dp.init_from_env()
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a HIP device (poweflownet_amd has no CPU fallback)")
    dist_on = dp.active()                # world > 1 (or PFN_FORCE_DIST=1: the collective path on a one-GPU box)
    if world != args.gpus:               # a 1-GPU number must never be labelled as an N-GPU one (or the reverse)
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    dev = torch.device("cuda", local_rank)
    h, Lg, K = CONFIGS[args.config]
    torch.manual_seed(1234)                           # train.py:70 -> identical replicas on every rank
    model = MaskEmbdMultiMPN(4, 2, 4, h, Lg, K, 0.2).to(dev)
    model.seed_dropout(1234 + rank)
    data_cpu = make_batch(args.case, args.batch, seed=rank, hub_frac=args.hub_frac)
    data = data_cpu.to(dev)
    n_nodes = data.x.shape[0]
    train = args.mode == "train"
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    masked = args.loss == "masked_l2"
    loss_fn = Masked_L2_loss() if masked else MSELoss()   # MSELoss: torch.nn.MSELoss semantics (train.py:103), fwd+bwd in one pass
    loss_box = [None]
    out_box = [None]         # the model's prediction of the last step (--dump-outputs); in training, written by the backward pass

    if train:
        model.train()
        from poweflownet_amd.optim import FlatAdamW
        opt = FlatAdamW(model, lr=1e-3)               # AdamW (train.py:123) as one HIP kernel on the flat buffers

        def fwd_bwd():
            opt.zero_grad(set_to_none=True)
            # the loop body's promise (utils/training.py:59-74): the loss, then its backward
            if masked:
                loss_fn.attach(model, data.y, data.pred_mask)
            else:
                loss_fn.attach(model, data.y)
            out = model(data)
            loss = loss_fn(out, data.y, data.pred_mask) if masked else loss_fn(out, data.y)
            loss.backward(loss_fn.unit_grad(loss))     # == loss.backward(), minus autograd's ones_like + mul kernels
            loss_box[0] = loss
            out_box[0] = out.detach()

        def step_eager():
            fwd_bwd()
            dp.allreduce_gradients(model)
            opt.step()
    else:
        model.eval()

        def step_eager():
            with torch.no_grad():
                loss_box[0] = out_box[0] = model(data)

    # ---- warm-up on a side stream (builds the topology cache, autotunes nothing, primes the allocator)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step_eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    directed, e_eff = model._graphs._graph.info()
    # what a step changes (parameters, AdamW moments and step count, the dropout stream's offset): kept as the warm-up left it,
    # and put back in place right before the timed steps, which therefore compute the same values however many ramp steps ran
    state = [t for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_count, model._rng_state) if t is not None] \
        if train else []
    saved = [t.clone() for t in state]

    use_graph = not args.no_graph
    launch_mode = "eager"
    if use_graph:
        try:
            if train:
                opt.zero_grad(set_to_none=True)

                def fb():
                    fwd_bwd()
                    return loss_box[0]
                # ONE hipGraph per step: forward, loss, backward, (DP: the RCCL all-reduce of the flat gradient buffer, captured
                # between backward and optimizer like any other node; a backend that cannot be captured -- gloo in the one-GPU
                # plumbing tests -- gets graph / eager all-reduce / graph), AdamW
                gs = dp.GraphedStep(fb, opt.step, model, mode=args.dp_mode).capture()
                step, launch_mode = gs.replay, ("hipGraph replay: " if gs.form != "eager" else "") + gs.mode
            else:
                g_inf = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_inf):
                    step_eager()
                step, launch_mode = g_inf.replay, "hipGraph replay: one graph"
        except Exception as exc:                  # noqa: BLE001  (a capture that fails must not take the run down)
            print(f"rank {rank}: hipGraph capture failed ({exc}); running eager", file=sys.stderr)
            torch.cuda.synchronize()
            use_graph = False
            step = step_eager
    else:
        step = step_eager

    def barrier():
        if dist_on:
            torch.distributed.barrier()

    # ---- clock ramp: untimed, in addition to (and before) the W warm-up steps the contract asks for.  The step count is fixed
    # by rank 0 from eight probe steps and broadcast, so every rank issues the same sequence of collectives
    ramp_steps = 0
    if args.clock_ramp_ms > 0:
        torch.cuda.synchronize()
        barrier()
        t_ramp = time.perf_counter()
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        est = max((time.perf_counter() - t_ramp) / 8, 1e-6)
        more = max(0, min(int(1e-3 * args.clock_ramp_ms / est) - 8, 20000))
        if dist_on:
            t = torch.tensor([more], device=dev, dtype=torch.int64)
            torch.distributed.broadcast(t, src=0)
            more = int(t.item())
        for _ in range(more):
            step()
        ramp_steps = 8 + more
    for _ in range(args.warmup):
        step()
    for t, t0 in zip(state, saved):
        t.copy_(t0)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    own_elapsed = elapsed
    if dist_on:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / args.steps
    value = args.batch * world * args.steps / elapsed
    ranks_info = rank_roster(dev, local_rank, 1e3 * own_elapsed / args.steps, world, dist_on)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"output": out_box[0], "loss": loss_box[0], "params": opt.flat_param} if train
                     else {"output": out_box[0]})
    median_ms = min_ms = None
    if args.full:
        # the same K steps once more with one event per step boundary: median / min step time (SURVEY 8d asks for the median;
        # the contract's timed region above stays free of event records, each of which costs a few microseconds on the stream)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        evs[0].record()
        for i in range(args.steps):
            step()
            evs[i + 1].record()
        torch.cuda.synchronize()
        barrier()
        per_step = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
        median_ms = per_step[len(per_step) // 2] if len(per_step) % 2 else 0.5 * (per_step[len(per_step) // 2 - 1] + per_step[len(per_step) // 2])
        min_ms = per_step[0]
    final = loss_box[0]
    final_loss = float(final.float().mean().item()) if final is not None else None

    # ---- per-kernel timing pass (eager, HIP events on the launch stream) -> roofline of the dominant kernel
    roofline, kernels, step_flops = None, {}, None
    profile_steps = args.profile_steps if args.full else 0
    if profile_steps > 0:
        # every rank runs the eager steps (they contain the gradient all-reduce: a rank that skipped them would leave the
        # others waiting in the collective); only rank 0 records and reports
        # one untimed eager step first: the eager pass allocates its own workspaces (the replayed step's live in the graph's
        # private pool), and kernels that touch freshly mapped memory for the first time run long -- with two profiled steps
        # the table of case118v2 x 2048 summed to 1.10 x the step it describes
        step_eager()
        torch.cuda.synchronize()
        if rank == 0:
            L.profile_report(reset=True)
            L.profile_enable(True)
        for _ in range(profile_steps):
            step_eager()
        torch.cuda.synchronize()
        barrier()
    if rank == 0 and profile_steps > 0:
        L.profile_enable(False)
        rep = L.profile_report(reset=True)
        ab = alg_bytes(n_nodes, e_eff, h, 2, K, train)
        # beyond 32,768 rows the first layer's P | Q are formed in the edge walk from x0 (inference; training whose backward
        # walks read saved masks, i.e. when the graph-resident backward kernels are not in use): model.hip first_layer_fly
        l0_fly = n_nodes > 32768 and (not train or "ea_seg_bwd" not in rep)
        # every event-pair interval has had the live-measured interval of an EMPTY pair subtracted by the library
        event_pair_overhead_us = round(1e3 * rep.pop("__event_pair_overhead", {"ms": 0.0})["ms"], 3)
        step_flops = 0.0
        for name, r in rep.items():
            cnt = max(r["count"], 1)
            avg_s = max(1e-3 * r["ms"] / cnt, 1e-9)   # (a kernel shorter than the subtracted event-pair overhead reads 0)
            row = {"launches_per_step": r["count"] / args.profile_steps, "avg_us": round(1e6 * avg_s, 3),
                   "ms_per_step": round(r["ms"] / args.profile_steps, 4)}
            step_flops += r["flops"] / args.profile_steps
            if name in ab:
                nbytes = ab[name]
                if name in ("edge_fwd", "edge_rows_fwd") and l0_fly:
                    # the first layer's launch reads 16-byte x0 rows where the others read (gather) H-wide P / Q rows: its own
                    # smaller byte count enters the class average, not the H-wide one
                    launches_ps = r["count"] / args.profile_steps
                    first = nbytes - 4.0 * (n_nodes * h + (n_nodes if name == "edge_rows_fwd" else e_eff) * h) \
                        + 4.0 * (4 * n_nodes + (0 if name == "edge_rows_fwd" else 4 * e_eff))
                    nbytes = (nbytes * (launches_ps - 1) + first) / max(launches_ps, 1)
                row.update(bound="hbm", achieved=round(nbytes / avg_s / 1e9, 1), unit="GB/s",
                           frac=round(nbytes / avg_s / HBM_PEAK, 4), per_launch=nbytes)
                if name.startswith("fused_hops"):
                    # what K separate hop launches would have moved (K x B_sa(H)) over this kernel's time: NOT a roofline fraction
                    row["equiv_unfused_GBps"] = round(K * ab["hop_norm"] / avg_s / 1e9, 1)
            elif r["flops"] > 0:
                fl = r["flops"] / cnt
                row.update(bound="mfma", achieved=round(fl / avg_s / 1e12, 2), unit="TFLOP/s",
                           frac=round(fl / avg_s / MFMA_F32_PEAK, 4), per_launch=fl)
                if r.get("bytes", 0) > 0:
                    # the same launches against the OTHER roof: their algorithmic operand + output bytes over the same time.  A class
                    # whose two fractions are comparable sits at the ridge (gemm_nt's one-piece products at large M: DESIGN.md
                    # section 9) -- neither roof alone bounds it
                    by = r["bytes"] / cnt
                    row.update(hbm_side_bytes_per_launch=by, hbm_side_frac=round(by / avg_s / HBM_PEAK, 4),
                               flop_per_byte=round(fl / by, 1), ridge_flop_per_byte=round(MFMA_F32_PEAK / HBM_PEAK, 1))
            kernels[name] = row
        rated = {k: v for k, v in kernels.items() if "bound" in v}
        if rated:
            dom = max(rated, key=lambda k: rated[k]["ms_per_step"])
            d = rated[dom]
            roofline = {"kernel": dom, "bound": d["bound"], "achieved": d["achieved"],
                        "peak": HBM_PEAK / 1e9 if d["bound"] == "hbm" else MFMA_F32_PEAK / 1e12, "unit": d["unit"],
                        "frac": d["frac"], "traffic": None, "avg_launch_us": d["avg_us"],
                        "launches_per_step": d["launches_per_step"],
                        "algorithmic_per_launch": d["per_launch"],
                        "event_pair_overhead_us_subtracted": event_pair_overhead_us}
            if not args.no_live_traffic and world == 1:
                t, detail = live_traffic(args, dom)
                if t is not None:
                    roofline["traffic"], roofline["traffic_source"] = t, "rocprofv3 --pmc passes run by this bench.py invocation"
                    roofline["traffic_detail"] = detail
                else:
                    roofline["traffic_note"] = detail
            tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
            if roofline["traffic"] is None and os.path.exists(tfile):
                try:
                    key = f"{dom}:{args.case}:{args.batch}:{args.mode}"
                    if args.config != "standard":
                        key += ":" + args.config
                    if args.hub_frac > 0:
                        key += f":hub{args.hub_frac}"
                    t = json.load(open(tfile)).get(key)
                    if t is not None:
                        # fallback: the figure tools/profile_round.sh recorded for this workload in an earlier session
                        roofline["traffic"] = t
                        roofline["traffic_source"] = "profiles/pmc_traffic.json (recorded earlier, not in this run)"
                except Exception:
                    pass

    # ---- SURVEY 8(d) extras (single GPU, training): the optimiser-free step, and a step with a COLD topology cache (a new
    # edge_index tensor: adjacency rebuilt on device, one host sync for the id-range check), both eager-launched
    extras = {}
    if rank == 0 and world == 1 and not train and not args.child and args.full:
        def timed_inf(fn, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / reps
        extras["eager_ms_per_step"] = round(timed_inf(step_eager, 10 if ms_per_step > 5.0 else 100), 4)
        if args.batch == 1:
            # the reference's own latency loop (perfomance_evaluator.py:61-74): model(sample) per sample, batch of one
            extras["latency_us_per_sample"] = {"hipGraph_replay": round(1e3 * median_ms, 2), "eager_launches": round(1e3 * extras["eager_ms_per_step"], 2)}
    if rank == 0 and world == 1 and train and not args.child and args.full:
        def timed(fn, reps):
            """ms per call: the best of three loops of `reps` pipelined calls (one untimed call first: first-use allocations of
            this stream's memory pool; best-of-three: a one-off allocator or driver hiccup of ~0.3 s inside a 10-call loop was
            reported as 44 instead of 14 ms per step)."""
            fn()
            best = None
            for _ in range(3 if reps > 1 else 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                dt = 1e3 * (time.perf_counter() - t0) / reps
                best = dt if best is None else min(best, dt)
            return best
        reps_e = 10 if ms_per_step > 5.0 else 100            # (a short loop mostly measures the fill and drain of the launch queue)

        def on_side(fn):
            # Eager launches on the stream the warm-up ran on: autograd binds every parameter's gradient accumulator to the
            # stream of its FIRST backward (here the warm-up's side stream -- a capture needs one), and a backward on any other
            # stream pays an event record + wait per parameter on the host (35 of them: 1.06 instead of 0.69 ms per step)
            def run():
                with torch.cuda.stream(side):
                    fn()
            return run
        side.wait_stream(torch.cuda.current_stream())
        extras["eager_ms_per_step"] = round(timed(on_side(step_eager), reps_e), 4)
        extras["eager_fwd_bwd_only_ms"] = round(timed(on_side(fwd_bwd), reps_e), 4)
        extras["eager_other_stream_ms_per_step"] = round(timed(step_eager, reps_e), 4)
        ei_saved = data.edge_index

        flip = [0]

        from poweflownet_amd.networks.MPN import _GraphCache

        def cold():
            # a topology met for the FIRST time (an empty adjacency cache): build on the device + the validating read-backs (ids in
            # range, the batch a union of equal graphs) -- the one place a forward synchronises with the host
            flip[0] ^= 1
            data.edge_index = ei_saved.flip(1).contiguous() if flip[0] else ei_saved.clone().roll(1, 1).contiguous()
            model._graphs = _GraphCache()
            fwd_bwd()
        reps = [timed(cold, 1) for _ in range(5)]
        extras["cold_topology_fwd_bwd_ms"] = round(sorted(reps)[len(reps) // 2], 4)       # median of 5
        extras["cold_topology_reps_ms"] = [round(r, 3) for r in reps]
        data.edge_index = ei_saved
        fwd_bwd()

        def same_content():
            # what a PyG-style loader hands out (train.py:90-92): a NEW tensor, the SAME edges -> rebuilt on the device, checks
            # left there, no host sync (round 5 compared contents and read the verdict back: 1.14 ms)
            data.edge_index = ei_saved.clone()
            fwd_bwd()
        same_content()
        reps = [timed(on_side(same_content), 1) for _ in range(5)]
        extras["same_content_new_tensor_fwd_bwd_ms"] = round(sorted(reps)[len(reps) // 2], 4)
        extras["same_content_new_tensor_pipelined_ms"] = round(timed(on_side(same_content), reps_e), 4)   # 100 calls, one sync
        data.edge_index = ei_saved
        fwd_bwd()
        # ---- the reference's OWN loop shape, nothing of this package's training plumbing: torch.nn.MSELoss,
        # torch.optim.AdamW(model.parameters()), eager launches, a NEW Batch object (new tensors) per step, no attach(), no
        # FlatAdamW, no hipGraph -- utils/training.py:55-77 + train.py:103,123 line by line, incl. its per-batch loss.item()
        try:
            torch.manual_seed(1234)
            m_ref = MaskEmbdMultiMPN(4, 2, 4, h, Lg, K, 0.2).to(dev)
            m_ref.seed_dropout(1234)
            m_ref.train()
            opt_ref = torch.optim.AdamW(m_ref.parameters(), lr=1e-3)
            lf_ref = torch.nn.MSELoss()
            acc = [0.0]

            def ref_body(item):
                d = data.clone()                      # `for data in loader: data = data.to(device)`: a new Batch, new tensors
                opt_ref.zero_grad()
                out = m_ref(d)
                loss = lf_ref(out, d.y)
                loss.backward()
                opt_ref.step()
                if item:
                    acc[0] += loss.item() * len(d)    # utils/training.py:76-77: a host sync per batch
            for _ in range(5):
                ref_body(True)
            extras["ref_loop_ms_per_step"] = round(timed(on_side(lambda: ref_body(True)), reps_e), 4)
            extras["ref_loop_no_item_ms_per_step"] = round(timed(on_side(lambda: ref_body(False)), reps_e), 4)
            extras["ref_loop"] = ("utils/training.py:55-77 as written: torch.nn.MSELoss + torch.optim.AdamW(model.parameters()) + eager "
                                  "launches + a new Batch per step + loss.item() per step; `no_item`: the same without the per-step read-back")
            del m_ref, opt_ref
        except Exception as exc:                  # noqa: BLE001
            extras["ref_loop_error"] = f"{type(exc).__name__}: {exc}"[:300]
        if use_graph and not dist_on and not args.no_dp_overhead:
            extras.update(dp_overhead(fb, opt, model, dev, args.steps, ms_per_step))
        if use_graph and not dist_on:
            # a topology that changes per batch (the reference's `perturbed` datasets): the adjacency build -- is_directed,
            # undirect, both CSRs, degrees, the segment check -- is INSIDE the replayed graph, nothing syncs with the host
            try:
                model.dynamic_topology = True
                side2 = torch.cuda.Stream()
                side2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side2):
                    step_eager()
                torch.cuda.current_stream().wait_stream(side2)
                torch.cuda.synchronize()
                opt.zero_grad(set_to_none=True)
                gdyn = dp.GraphedStep(fb, opt.step, model, allreduce=False).capture()
                extras["dynamic_topology_ms_per_step"] = round(timed(gdyn.replay, max(10, args.steps)), 4)
                del gdyn
            except Exception as exc:              # noqa: BLE001
                extras["dynamic_topology_error"] = f"{type(exc).__name__}: {exc}"[:300]
            finally:
                model.dynamic_topology = False

    # ---- the scatter-add in isolation (north_star's 40 % figure): pfn_scatter_add over this batch's adjacency, F = hidden_dim,
    # against B_sa(F) = 4 [E F + E + N F + (N+1)]; HIP events on the launch stream around 20 back-to-back launches
    scatter = None
    if rank == 0 and not args.child and args.full:
        gws = model._graphs._graph
        xs = torch.randn(n_nodes, (h + 3) // 4 * 4, device=dev)
        xs[:, h:] = 0
        ys = torch.empty_like(xs)
        lib = L.load()

        def sa():
            L.check(lib.pfn_scatter_add(gws.ws.data_ptr(), n_nodes, gws.e_stored, xs.data_ptr(), ys.data_ptr(), h,
                                        L.stream_ptr()), "pfn_scatter_add")
        for _ in range(3):
            sa()
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            sa()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        b_sa = 4.0 * (e_eff * h + e_eff + n_nodes * h + (n_nodes + 1))
        ws_mb = (2 * xs.numel() * 4 + 4 * (e_eff + n_nodes)) / 2**20
        scatter = {"kernel": "pfn_scatter_add (hop_kernel<false>)", "F": h, "us": round(us, 2),
                   "regime": ("cache-warm: %d back-to-back launches on one %.0f MiB working set (<= the 256 MiB Infinity Cache); "
                              "the in-step figure is kernels.hop_norm where that kernel runs" % (reps, ws_mb)) if ws_mb <= 256 else
                             ("HBM: the %.0f MiB working set exceeds the 256 MiB Infinity Cache" % ws_mb),
                   "algorithmic_bytes": b_sa, "achieved": round(b_sa / (us * 1e-6) / 1e9, 1), "unit": "GB/s",
                   "frac": round(b_sa / (us * 1e-6) / HBM_PEAK, 4), "launches_timed": reps}
        del xs, ys
    barrier()

    bytes_step = b_fwd(n_nodes, e_eff, h, Lg, K) * (3.0 if train else 1.0)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.full:
        cpu = cpu_baseline(args, (h, Lg, K), data_cpu, args.cpu_seconds)

    others = None
    if rank == 0 and world == 1 and not args.child and args.full and not args.no_other_configs and train and str(args.case) == "118v2" \
            and args.batch == 128 and args.config == "standard" and not under_profiler():
        del data, model                                # (the children need the memory more than this process does from here on)
        torch.cuda.empty_cache()
        others = other_configs()

    if rank == 0:
        n_case, e_case = CASES[str(args.case)]
        # a fraction above 1 is a broken denominator, not a fast kernel: never print one
        bad = [k for k, v in kernels.items() if v.get("frac") is not None and v["frac"] > 1.0]
        for k in bad:
            kernels[k]["frac_rejected"] = kernels[k].pop("frac")
        if scatter is not None and scatter["frac"] > 1.0:
            scatter["frac_rejected"] = scatter.pop("frac")
            bad.append("scatter_add")
        # the per-kernel table must not add up to more than the step it describes (the eager profiling pass and the replayed
        # step run the same kernels): a table that does is not evidence for any of its rows
        kernels_sum_ms = round(sum(v["ms_per_step"] for v in kernels.values()), 4) if kernels else None
        if kernels_sum_ms is not None and kernels_sum_ms > 1.03 * ms_per_step:
            bad.append(f"kernel_table_sum {kernels_sum_ms} ms > 1.03 x ms_per_step {round(ms_per_step, 4)}")
        if roofline is not None and roofline["frac"] > 1.0:
            sys.exit(f"bench.py: roofline fraction {roofline['frac']} > 1 for {roofline['kernel']}: broken denominator")
        out = {
            "metric": f"graphs/sec {'fwd+bwd (train step incl. AdamW)' if train else 'inference fwd'}, "
                      f"case{args.case} batch={args.batch}",
            "value": round(value, 1), "unit": "graphs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "clock_ramp_steps": ramp_steps,
            "ms_per_step": round(ms_per_step, 4), "median_ms_per_step": None if median_ms is None else round(median_ms, 4),
            "min_ms_per_step": None if min_ms is None else round(min_ms, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"case{args.case} ({n_case} buses, {e_case} branches, synthetic topology) "
                                   f"MaskEmbdMultiMPN {args.config}.json (H{h} L{Lg} K{K} dropout 0.2) "
                                   f"{'training step fwd+MSELoss+bwd+AdamW' if train else 'eval forward'}, fp32",
                       "graphs_per_gpu": args.batch, "global_batch": args.batch * world, "nodes_per_gpu": n_nodes,
                       "directed_edges_per_gpu": e_eff, "parallelism": f"dp{world}",
                       "launch": launch_mode, "undirected_on_device": directed,
                       "hub_frac": args.hub_frac},
            "step_algorithmic_bytes": bytes_step,
            "step_hbm_frac": round(bytes_step / (1e-3 * ms_per_step) / HBM_PEAK, 4),
            "step_gemm_flops": step_flops,
            "step_mfma_frac": None if not step_flops else round(step_flops / (1e-3 * ms_per_step) / MFMA_F32_PEAK, 4),
            "fractions_rejected": bad, "kernels_sum_ms_per_step": kernels_sum_ms,
            "final_loss": final_loss, **ranks_info, **extras,
            "roofline": roofline, "scatter_add": scatter, "cpu_baseline": cpu, "kernels": kernels,
        }
        if others is not None:
            out["other_configs"] = others
        if cpu:
            out["speedup_vs_cpu"] = round(value / cpu["value"], 1)
        print(json.dumps(out))
    if dist_on:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
