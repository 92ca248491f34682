"""bench.py - edges/s of the SegmentClassifier forward on synthetic TrackML-shaped graphs.

    python bench.py --gpus N --steps K --warmup W [--workload c3|c5] [--full] [--dump-outputs DIR]

One "step" = one pass of the hot path (input network, T x (edge pass, node pass), final
edge pass; reference gnn/model.py:140-156) over one batch of G synthetic graphs already
resident in HBM, in index form.  Default workload = BASELINE.json configs[2] ("c3"): 10k
hits / 100k segments per graph, F=3, D=8, T=3, G graphs per launch per GPU (SURVEY.md 8(d):
one 100k-segment graph is cache-resident and launch-bound, so the roofline number is taken
on a batch).  `--workload c5` = configs[4]: 50k hits / 500k segments, D=64, T=6, G=8, bf16
matrix-core hit update (fp32 beside it), with the MFMA fraction next to the HBM fraction.

Multi-GPU: independent graphs sharded over ranks, no data-path collective in the forward
(weak scaling); barrier + synchronize on both sides, max over ranks.  `--gpus N` with N > 1
and no torchrun environment starts the N ranks itself (child processes of a parent that
never touches the GPU) and relays rank 0's line.

A plain run sets up, warms up, times exactly K steps (one region, no retries), writes the last
step's outputs if --dump-outputs DIR is given, and prints ONE JSON line: metric, value (edges/s over
the K steps), unit, higher_is_better, dtype, ms_per_step (one timed step), the run's config.

--dump-outputs DIR: the edge scores the last timed step returned (rank 0's graphs) as DIR/scores.npy,
float32; beyond 2^23 segments a fixed sample of them (numpy seed 0, ascending segment index).  Graphs
and weights are seeded, so two builds given the same arguments can be compared score for score.

--full adds to the same line (each in runs of its own, after the timed steps):
  roofline      dominant kernel, HIP-event timed inside the library on the launch stream: a pass of
                >= 3 x K forwards, the first third dropped, MEDIAN per launch position; the sum of the
                medians must not exceed 1.05 x ms_per_step (`consistent`)
  value_exact_exp  the same forward with the exp-product mode off (what trained weights outside
                its proven range run)
  c5            (N = 1, c3) BASELINE configs[4]: 8 x (50k hits, 500k segments), D=64, T=6, exact fp32
                and bf16 records, with the dominant kernel's HBM fraction and committed counters
  cpu_baseline  the oracle's dense-bmm port of the reference algorithm on this host (N=1 only)
  train_c3      (N = 1, c3) one training step on 32 of the workload's graphs as one batch
  plan_ms       what the per-batch execution plan costs (outside the timed region), and the
                rate of one forward on a FRESH batch, plan included (`value_incl_plan`)
  train_c4      BASELINE configs[3]: 512 muon graphs sharded r::N, HIP forward + fused BCE +
                HIP backward + ONE all-reduce of the flat gradient bucket (RCCL) + Adam
                (reference gnn/estimator.py:49-60)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

DUMP_SAMPLE = 1 << 23    # --dump-outputs: at most this many scores (32 MB of float32)
HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak
F32_MATRIX_TFLOPS = 157.3

WORKLOADS = {
    # name: hits, segments, F, D, T, default graphs per launch per GPU
    "c3": dict(n=10000, e=100000, F=3, D=8, T=3, G=256,
               text="c3 synthetic TrackML ACTS graphs: %d graphs/launch/GPU x (10k hits, 100k segments), "
                    "F=3, D=8, 3 MP iterations + final edge pass, index form resident in HBM"),
    "c5": dict(n=50000, e=500000, F=3, D=64, T=6, G=8,
               text="c5 mu200-shaped graphs: %d graphs/launch/GPU x (50k hits, 500k segments), F=3, "
                    "D=64, 6 MP iterations + final edge pass (gnn/MPNN_Seg_ACTS_mu200.ipynb cells 15, "
                    "19), index form resident in HBM"),
}


def algorithmic(n, e, F, D, T, w=4):
    """compulsory HBM bytes (w-byte values, int32 indices) and flops per kernel
    launch and for the whole forward."""
    C = F + D
    b_in = w * n * F + w * n * D
    b_edge = 8 * e + w * n * C + w * e
    b_node = 8 * e + w * e + w * n * C + w * n * D
    f_edge = e * (4 * C * D + 2 * D)
    f_agg = 4 * e * C
    f_node = n * (6 * C * D + 2 * D * D)
    f_in = 2 * n * F * D
    it_b, it_f = b_edge + b_node, f_edge + f_agg + f_node
    return {"bytes": {"k_input": b_in, "k_input4": b_in, "k_edge": b_edge, "k_node": b_node, "k_iter": it_b,
                      "k_iter_w": it_b, "k_iter_wx": it_b, "k_iter2": it_b, "k_pack": 0, "k_pack16": 0,
                      "forward": b_in + (T + 1) * b_edge + T * b_node},
            "flops": {"k_input": f_in, "k_input4": f_in, "k_edge": f_edge, "k_node": f_agg + f_node,
                      "k_iter": it_f, "k_iter_w": it_f, "k_iter_wx": it_f, "k_iter2": it_f, "k_pack": 0, "k_pack16": 0,
                      "forward": f_in + (T + 1) * f_edge + T * (f_agg + f_node)}}


def cpu_baseline(model, graph, wl):
    """Oracle timed on this host: (a) the dense-bmm port of reference gnn/model.py (the
    algorithm the reference runs), one c3 graph; (b) the index-form C oracle, all cores.
    c5: the dense form needs 100 GB per incidence matrix - index form only."""
    import torch
    from oracle import dense_torch, index_c
    from gnn_fpga_amd import synth
    # the GPU box gives one GPU a 16-CPU share of a 256-thread host: do not oversubscribe
    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    pn = {k: v.numpy() for k, v in params.items()}
    T, e = wl["T"], wl["e"]
    index_c.segment_classifier(graph.X, graph.src, graph.dst, pn, T, n_threads=cores)  # warm
    reps = 20 if e <= 100000 else 3
    t0 = time.perf_counter()
    for _ in range(reps):
        index_c.segment_classifier(graph.X, graph.src, graph.dst, pn, T, n_threads=cores)
    t_index = (time.perf_counter() - t0) / reps
    idx_sample = ("1 graph of the workload, index-form restatement oracle/index_c (OpenMP, %d threads), "
                  "mean of %d runs" % (cores, reps))
    if wl["n"] * wl["e"] > 2e9:
        return {"value": e / t_index, "unit": "edges/s", "cores": cores, "kind": "port",
                "sample": idx_sample + "; the reference's dense [N,E] formulation cannot run at this "
                                        "size (100 GB per incidence matrix)"}
    X, Ri, Ro = (torch.from_numpy(a)[None] for a in synth.to_dense(graph))
    t0 = time.perf_counter()
    with torch.no_grad():
        dense_torch.segment_classifier(X, Ri, Ro, params, T)
    t_dense = time.perf_counter() - t0
    return {"value": e / t_dense, "unit": "edges/s", "cores": cores, "kind": "port",
            "sample": "1 graph of the workload (10k hits, 100k segments), dense [N,E] bmm "
                      "formulation of gnn/model.py restated in oracle/dense_torch.py, "
                      "torch CPU %d threads, 1 run (%.1f s)" % (cores, t_dense),
            "index_form_value": e / t_index, "index_form_sample": idx_sample}


def event_medians(step, steps):
    """Per-launch kernel times of one step: HIP events recorded by the library around every launch, on
    the launch stream, in a pass of its own (events perturb a timed region).  The pass runs n >= 3 x
    `steps` (>= 30) steps; the first third is dropped (event creation idles the GPU: the clocks ramp
    again) and every launch POSITION of a step gets the MEDIAN of the rest.
    -> [(kernel_name, median_ms), ...] in launch order."""
    from gnn_fpga_amd import _lib
    n = min(max(3 * steps, 30), 600)
    with _lib.profile(capacity=40 * n) as prof:
        for _ in range(n):
            step()
    lps = len(prof.records) // n
    if lps == 0 or lps * n != len(prof.records):
        return []
    out = []
    for i in range(lps):
        v = sorted(prof.records[k * lps + i][1] for k in range(n // 3, n))
        out.append((prof.records[i][0], v[len(v) // 2]))
    return out


def pmc_section(path, key):
    """Committed counter record of one workload (profiles/pmc_traffic.json, written by
    tools/make_pmc_traffic.py from separate rocprofv3 --pmc passes), or None."""
    if not (path and os.path.exists(path)):
        return None
    with open(path) as f:
        pj = json.load(f)
    sec = pj if key == "c3" and "kernels" in pj else pj.get(key)
    return sec if sec and "kernels" in sec else None


def kernel_traffic(sec, kernel):
    """Launch-weighted HBM bytes per launch over the template variants of `kernel`."""
    vs = [v for k, v in sec["kernels"].items() if k.split("<")[0] == kernel]
    if not vs:
        return None
    return (sum(v["hbm_bytes_per_launch"] * v.get("launches", 1) for v in vs) /
            sum(v.get("launches", 1) for v in vs))


def c5_record(dev, steps, pmc_path, G=8):
    """BASELINE configs[4] inside the default line (N = 1): G x (50k hits, 500k segments), D = 64,
    T = 6 (gnn/MPNN_Seg_ACTS_mu200.ipynb cells 15, 19), exact fp32 records (the default wide path)
    and bf16 records / bf16 matrix-core products (BASELINE's dtype for this config; scores within
    2e-3, not 1e-5).  The bound reported is the one the kernels are actually against: HBM bytes of the
    dominant kernel (`k_iter_w`) - algorithmic, and measured (`traffic`, committed PMC passes) - with
    the vector-ALU busy fraction beside it; the per-segment-contraction MFMA figure of earlier rounds
    was nominal (the kernels run the per-hit form, 10x fewer multiply-adds) and is gone."""
    import torch
    from gnn_fpga_amd import HitGraphBatch, synth
    from gnn_fpga_amd.model import SegmentClassifier
    wl = WORKLOADS["c5"]
    n, e, F, D, T = wl["n"], wl["e"], wl["F"], wl["D"], wl["T"]
    graphs = [synth.layered_graph(n, e, F, seed=1000 + i) for i in range(G)]
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    torch.manual_seed(0)
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).to(dev).eval()
    model.use_events = False
    K = max(steps // 2, 10)
    rec = {"workload": wl["text"] % G, "steps": K}
    with torch.no_grad():
        for bf16 in (False, True):
            model.mlp_bf16 = bf16
            step = lambda: model(batch)          # noqa: E731
            for _ in range(10):
                step()
            dt = time_steps(step, K, torch.cuda.synchronize) / K
            seq = event_medians(step, K)
            tag = "bf16" if bf16 else "f32"
            sub = {"ms_per_step": dt * 1e3, "value": batch.n_segments / dt, "unit": "edges/s"}
            per = {}
            for name, ms in seq:
                per.setdefault(name, []).append(ms)
            if per:
                dom = max(per, key=lambda k: sum(per[k]))
                alg = algorithmic(batch.n_hits, batch.n_segments, F, D, T, w=2 if bf16 else 4)
                t_dom = sum(per[dom]) / len(per[dom]) * 1e-3
                ab = alg["bytes"].get(dom, alg["bytes"]["k_iter_w"])
                sub.update({"kernel": dom, "avg_launch_ms": t_dom * 1e3,
                            "launches_per_step": len(per[dom]),
                            "algorithmic_bytes_per_launch": ab,
                            "hbm_achieved_GBps": ab / t_dom / 1e9,
                            "hbm_frac": ab / t_dom / 1e9 / HBM_PEAK_GBS,
                            "sum_kernel_ms": sum(ms for _, ms in seq),
                            "consistent": sum(ms for _, ms in seq) <= 1.05 * dt * 1e3,
                            "forward_frac": alg["bytes"]["forward"] / dt / 1e9 / HBM_PEAK_GBS})
                sec = pmc_section(pmc_path, "c5_" + tag)
                if sec:
                    tr = kernel_traffic(sec, dom)
                    sub["traffic"] = tr
                    sub["traffic_over_algorithmic"] = tr / ab if tr else None
                    sub["valu_busy"] = sec.get("valu_busy", {}).get(dom)
                    sub["counters_source"] = sec.get("source")
            rec[tag] = sub
    rec["bound"] = "hbm"
    rec["note"] = ("k_iter_wx (fp32) / k_iter_w (bf16): one launch per iteration; hbm_frac = SURVEY 8(d) B_edge + B_node of the "
                   "launch / its median time / 8 TB/s; traffic = FETCH_SIZE x 2 + WRITE_SIZE of a committed "
                   "rocprofv3 --pmc pass; valu_busy = SQ_ACTIVE_INST_VALU x 4 / SQ_BUSY_CU_CYCLES there")
    return rec


def fresh_single_graph(dev, model, graph, D, reps=5):
    """What the reference's trigger-style use pays (gnn/Inference.ipynb cell 3: one graph in, scores
    out): a NEVER-SEEN single graph already on the device -> scores ready, wall clock with a
    synchronize, best of `reps` fresh batch objects (code objects and allocator warm).  `ms`: the
    model's default route for a first forward (use_plan = "auto": segment lists by gnn_csr_build +
    the per-module kernels, no plan); `plan_route`: the same with the plan built first."""
    import torch
    from gnn_fpga_amd import HitGraphBatch
    best = (float("inf"), 0.0, 0.0)
    first = float("inf")
    with torch.no_grad():
        for _ in range(reps + 1):
            b = HitGraphBatch.from_graphs([graph]).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(b)
            torch.cuda.synchronize()
            first = min(first, time.perf_counter() - t0)
        for _ in range(reps + 1):
            b = HitGraphBatch.from_graphs([graph]).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.build_plan(D)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            model(b)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if t2 - t0 < best[0]:
                best = (t2 - t0, t1 - t0, t2 - t1)
    # BASELINE configs[1]: one never-seen muon event (gnn/prepareMuonGraphs.py sizes, F = 11) to its scores - one
    # k_event launch that builds the event's segment lists in LDS itself; median of 50 fresh batch objects
    from gnn_fpga_amd import synth
    from gnn_fpga_amd.model import SegmentClassifier
    mm = SegmentClassifier(input_dim=11, hidden_dim=8, n_iters=3).to(dev).eval()
    mg = synth.muon_graph(3)
    ts = []
    with torch.no_grad():
        for _ in range(60):
            b = HitGraphBatch.from_graphs([mg]).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mm(b)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    muon_us = sorted(ts[10:])[25] * 1e6
    return {"ms": first * 1e3,
            "c2_muon_event_us": muon_us,
            "plan_route": {"ms": best[0] * 1e3, "plan_ms": best[1] * 1e3, "forward_ms": best[2] * 1e3},
            "what": "one never-seen graph of the workload, resident on the device, to its scores: synchronised "
                    "wall clock, best of %d; ms = the default first-forward route (gnn_csr_build + per-module "
                    "kernels, no plan), plan_route = plan build + fused forward; c2_muon_event_us = one never-seen muon event "
                    "(F = 11, ~20 hits) to its scores, one launch, median of 50" % reps}


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args):
    """`python bench.py --gpus N` without a torchrun environment: this parent has made NO GPU call
    (importing torch is not one); it starts the N ranks as children through torch.distributed.run,
    relays their output (rank 0 prints the JSON line) and exits with their code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "4")
    sys.stderr.write("bench.py: starting %d ranks: %s\n" % (args.gpus, " ".join(cmd)))
    return subprocess.call(cmd, env=env)


def time_steps(step, steps, sync_all, last=None):
    """Wall clock of `steps` calls of step(); `last` (a list) receives what the final call returned."""
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = step()
    sync_all()
    dt = time.perf_counter() - t0
    if last is not None:
        last.append(res)
    return dt


def dump_outputs(path, scores):
    """--dump-outputs: the scores one timed step returned, float32, as path/scores.npy - all of them up to
    DUMP_SAMPLE, else a fixed sample (numpy seed 0, ascending segment index).  -> what was written."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    s = scores.detach().reshape(-1).float().cpu().numpy()
    n = s.size
    if n > DUMP_SAMPLE:
        s = s[np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))]
    np.save(os.path.join(path, "scores.npy"), s)
    return {"scores": "%d of %d segment scores%s, float32" % (s.size, n, " (fixed sample, seed 0)" if s.size < n else "")}


def headline(args, wl, world, batch, plan, elapsed, bf16, G, dumped):
    """The line's headline fields (the whole line of a plain run): edges/s over the K timed steps."""
    out = {
        "metric": "edges/sec (EdgeNet+NodeNet fwd) on 100k-edge TrackML graphs; % HBM roofline",
        "value": world * batch.n_segments * args.steps / elapsed, "unit": "edges/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if bf16 else "f32",
        "data": "synthetic",
        "config": {"workload": wl["text"] % G,
                   "graphs_per_gpu": G, "hits_per_graph": wl["n"],
                   "segments_per_graph": wl["e"],
                   "plan": "hits relabelled by degree, SELL-16 lists (padding %.1f%%), built "
                           "once per batch on the GPU, outside the timed region like the CSR build "
                           "(plan_ms with --full)" % (100 * plan.padding),
                   "sharding": "independent graphs per rank, "
                   "no data-path collective"},
        "full": bool(args.full),
    }
    if dumped is not None:
        out["dumped_outputs"] = dumped
    return out


def train_c4(dev, rank, world, rehearse, steps=60, warmup=15, n_global=512):
    """BASELINE configs[3] as the ranks run it: 512 muon-schema graphs (F=11, D=8, T=3) sharded
    r::world, one training step = HIP forward (keeps e_t / H_t) + BCE(sum) + HIP backward into the
    flat GradBucket + ONE all-reduce of that bucket (RCCL over xGMI when world > 1) + Adam."""
    import torch
    import torch.distributed as dist
    from gnn_fpga_amd import HitGraphBatch, shard, synth
    from gnn_fpga_amd.loss import BCELoss
    from gnn_fpga_amd.model import SegmentClassifier
    graphs = shard.shard_graphs([synth.muon_graph(s) for s in range(n_global)], rank, world)
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    y = batch.y.to(dev)
    torch.manual_seed(0)
    m = SegmentClassifier(input_dim=11, hidden_dim=8, n_iters=3).to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
    bce = BCELoss(reduction="sum")
    bucket = shard.GradBucket(m.parameters())

    def step():
        bucket.zero()
        loss = bce(m(batch), y)             # local SUM; the all-reduce turns it into the global mean
        loss.backward()
        mean = bucket.allreduce(loss.detach(), y.numel())
        opt.step()
        return mean

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def step_direct():                      # the same step without an autograd graph (GradBucket.step)
        mean = bucket.step(m, batch, y)
        opt.step()
        return mean

    first = float(step())
    for _ in range(warmup):
        step()
    dt = time_steps(step, steps, sync_all)
    for _ in range(warmup):
        step_direct()
    dd = time_steps(step_direct, steps, sync_all)
    last = float(step())
    seg = torch.tensor([float(batch.n_segments), dt, dd], dtype=torch.float64, device=dev)
    if world > 1:
        segs = seg.clone()
        dist.all_reduce(segs, op=dist.ReduceOp.SUM)
        dist.all_reduce(seg, op=dist.ReduceOp.MAX)
        n_seg, dt, dd = float(segs[0]), float(seg[1]), float(seg[2])
    else:
        n_seg = float(seg[0])
    # did the collective see all ranks?  all-reduce of ones over the same backend
    ones = torch.ones(1, device=dev)
    if world > 1:
        dist.all_reduce(ones)
    rec = {"workload": "c4: %d muon-schema graphs (F=11, D=8, T=3) sharded r::%d, %d per rank"
                       % (n_global, world, len(graphs)),
           "us_per_step": dt / steps * 1e6, "segments_per_s": n_seg * steps / dt,
           "us_per_step_direct": dd / steps * 1e6, "segments_per_s_direct": n_seg * steps / dd,
           "direct": "GradBucket.step: same kernels and collective, no autograd graph (backward adds "
                     "straight into the bucket)",
           "segments_per_step": int(n_seg), "steps": steps,
           "collective": ("one all-reduce(sum) of the flat gradient bucket per step, %d floats, backend %s"
                          % (bucket.flat.numel(), ("gloo (rehearsal)" if rehearse else "nccl (RCCL)")
                             if world > 1 else "none (single rank)")),
           "rccl_ranks": int(ones.item()), "loss_first": first, "loss_last": last,
           "mode": "eager; us_per_step = the reference-style loop (forward, loss.backward(), bucket all-reduce, Adam)"}
    # the whole step as ONE captured HIP graph (the library launches on the capturing stream and
    # allocates nothing; Adam capturable).  With world > 1 the RCCL all-reduce sits INSIDE the capture
    # (the eager 8-rank step is host-launch-bound, not collective-bound); gloo (rehearsal) cannot be
    # captured.  A capture that raises falls back to the eager numbers above and says so.
    def capture():
        nonlocal opt
        try:
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True, fused=True)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step_direct()
            torch.cuda.current_stream().wait_stream(side)
            sync_all()
            cg = torch.cuda.CUDAGraph()
            # (thread-local capture mode with a collective inside: the RCCL watchdog thread's event
            # queries must not invalidate the capture)
            with torch.cuda.graph(cg, capture_error_mode="thread_local" if world > 1 else "global"):
                step_direct()
            for _ in range(warmup):
                cg.replay()
            dg = time_steps(cg.replay, steps, sync_all)
            if world > 1:
                t = torch.tensor([dg], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dg = float(t.item())
            rec["us_per_step_hip_graph"] = dg / steps * 1e6
            rec["segments_per_s_hip_graph"] = n_seg * steps / dg
            rec["hip_graph"] = ("GradBucket.step + Adam captured once and replayed%s"
                                % (", the RCCL all-reduce inside the capture" if world > 1 else ""))
        except Exception as ex:       # noqa: BLE001  (capture refused: the eager numbers stand)
            rec["hip_graph"] = "capture refused (%s: %s) - eager numbers only" % (type(ex).__name__, str(ex)[:120])

    if world > 1 and rehearse:
        rec["hip_graph"] = "gloo rehearsal: not capturable"
        return rec, None
    return rec, capture


def train_c3(dev, graphs, steps=30, warmup=8, hidden_dim=8, n_iters=3, n_graphs=32):
    """Training at the workload's graph size (N = 1 only): c3 - 32 of the graphs as one batch (3.2 M
    segments, D = 8, T = 3); c5 - one mu200-size graph with the model gnn/MPNN_Seg_ACTS_mu200.ipynb
    trains (D = 64, T = 6).  HIP forward that keeps e_t / H_t / Q_t + fused BCE + HIP backward + Adam,
    on the batch's level-ordered twin (hits in plan order, segments by end hit: built once)."""
    import torch
    from gnn_fpga_amd import HitGraphBatch, shard
    from gnn_fpga_amd.loss import BCELoss
    from gnn_fpga_amd.model import SegmentClassifier
    graphs = graphs[:n_graphs]
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    y = batch.y.to(dev)
    F = batch.X.shape[1]
    torch.manual_seed(0)
    m = SegmentClassifier(input_dim=F, hidden_dim=hidden_dim, n_iters=n_iters).to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
    bce = BCELoss()
    bucket = shard.GradBucket(m.parameters())

    def step():                              # the reference's loop (gnn/estimator.py:49-60)
        opt.zero_grad(set_to_none=False)
        loss = bce(m(batch), y)
        loss.backward()
        opt.step()
        return loss

    def step_direct():                       # no autograd graph: the backward adds into the bucket's views
        bucket.zero()
        loss = bucket.step(m, batch, y)
        opt.step()
        return loss

    sync = torch.cuda.synchronize
    first = float(step().detach())
    for _ in range(warmup):
        step()
    dt = time_steps(step, steps, sync)
    for _ in range(warmup):
        step_direct()
    dd = time_steps(step_direct, steps, sync)
    last = float(step().detach())
    n_seg = batch.n_segments
    rec = {"workload": "%d graph(s) of the workload as one batch (%d hits, %d segments), F=%d, D=%d, T=%d, BCE, Adam"
                       % (len(graphs), batch.n_hits, n_seg, F, hidden_dim, n_iters),
           "ms_per_step": dt / steps * 1e3, "segments_per_s": n_seg * steps / dt,
           "ms_per_step_direct": dd / steps * 1e3, "segments_per_s_direct": n_seg * steps / dd,
           "direct": "GradBucket.step: same kernels, no autograd graph, loss in the twin's segment order",
           "loss_first": first, "loss_last": last, "steps": steps}
    # the same step (GradBucket.step + Adam) captured once as a HIP graph and replayed: what its ~30 launches'
    # gaps are worth; a capture that raises leaves the eager numbers
    try:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True, fused=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step_direct()
        torch.cuda.current_stream().wait_stream(side)
        sync()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            step_direct()
        for _ in range(warmup):
            cg.replay()
        dg = time_steps(cg.replay, steps, sync)
        rec["ms_per_step_hip_graph"] = dg / steps * 1e3
        rec["segments_per_s_hip_graph"] = n_seg * steps / dg
    except Exception as ex:       # noqa: BLE001
        rec["hip_graph"] = "capture refused (%s: %s)" % (type(ex).__name__, str(ex)[:120])
    return rec


def run(args):
    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.dry_run:
        # the launch path alone (tests/test_bench_host.py, no GPU): rendezvous on 127.0.0.1, one
        # all-reduce over gloo, rank 0 prints a line, every rank leaves with code 0
        ones = torch.ones(1)
        if world > 1:
            dist.init_process_group("gloo")
            dist.all_reduce(ones)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dry_run": True, "ranks": int(ones.item()), "n_gpus": world}), flush=True)
        return
    # GNN_BENCH_REHEARSE=1: rehearsal of the N > 1 code path on a box with fewer GPUs than ranks
    # (ranks share devices, gloo instead of RCCL); the numbers of such a run mean nothing
    rehearse = os.environ.get("GNN_BENCH_REHEARSE") == "1"
    dev_index = local_rank % torch.cuda.device_count() if rehearse else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from gnn_fpga_amd import HitGraphBatch, _lib, synth
    from gnn_fpga_amd.model import SegmentClassifier

    wl = WORKLOADS[args.workload]
    N_HITS, N_SEG, F, D, T = wl["n"], wl["e"], wl["F"], wl["D"], wl["T"]
    G = args.graphs or wl["G"]
    bf16 = args.workload == "c5" and args.dtype != "f32"
    graphs = [synth.layered_graph(N_HITS, N_SEG, F, seed=rank * G + i) for i in range(G)]
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    limits = {"iter_records": 0, "edge_records": 0} if args.global_gather else None
    torch.cuda.synchronize()
    t_plan = time.perf_counter()
    plan = batch.build_plan(D, limits)     # relabel + SELL-16 lists: once per batch, like the CSR build
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t_plan
    torch.manual_seed(0)
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).to(dev).eval()
    model.use_events = False
    model.mlp_bf16 = bf16

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    with torch.no_grad():
        # one-off, before the W warm-up steps: first launches load the code objects, size the
        # workspace and let the clocks leave idle (a cold 1-ms step was seen to run 40 % long)
        # (K = 20 runs used to read 4 % slower than K = 100 ones: the clocks were still ramping)
        for _ in range(100 if args.workload == "c3" else 10):
            model(batch)
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            model(batch)
        step = lambda: model(batch)
        if args.graph:
            sync_all()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                graph_out = model(batch)
            step = lambda: (cg.replay(), graph_out)[1]      # noqa: E731  (the replay refills graph_out)
            step()
        last = []
        elapsed = time_steps(step, args.steps, sync_all, last)
        dumped = dump_outputs(args.dump_outputs, last[0]) if args.dump_outputs and rank == 0 else None
        del last
    if not args.full:
        if world > 1:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax[0].item())
        if rank == 0:
            print(json.dumps(headline(args, wl, world, batch, plan, elapsed, bf16, G, dumped)), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    with torch.no_grad():
        # per-kernel durations (see event_medians): a pass of its own, first third dropped, medians
        seq = event_medians(lambda: model(batch), args.steps)
        # A timed region that took much longer than its own kernels was not measuring them (seen once: 1.27 ms
        # per step over kernels of 0.85 when another process had just left the box).  One more region of
        # exactly K steps then, both on the record (`roofline.timed_regions_ms_per_step`); the headline stays
        # the first region.  Every rank takes the same branch (the decision is all-reduced) because sync_all
        # is a collective.
        timed_regions = [elapsed]
        retime = float(elapsed / args.steps * 1e3 > 1.15 * sum(ms for _, ms in seq) > 0.0)
        if world > 1:
            flag = torch.tensor([retime], dtype=torch.float64, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            retime = float(flag.item())
        if retime:
            timed_regions.append(time_steps(step, args.steps, sync_all))
        other = exact = None
        if args.workload == "c5":           # the other arithmetic beside it
            model.mlp_bf16 = not bf16
            for _ in range(2):
                model(batch)
            other = time_steps(step, max(args.steps // 4, 2), sync_all) / max(args.steps // 4, 2)
            model.mlp_bf16 = bf16
        elif not args.graph:
            # the exact-exp rate beside `value`: exp-product mode is only legal inside its proven range
            # (include/gnn_hip.h, GNN_FLAG_EXP_PRODUCT); weights outside it run this path
            model.exp_product = False
            ke = max(args.steps // 2, 10)
            for _ in range(5):
                model(batch)
            exact = time_steps(step, ke, sync_all) / ke
            model.exp_product = True
            model(batch)
        # the per-batch plan on the record: a second, fresh batch of the same graphs (code objects
        # and allocator warm), then one forward on it - what a stream of never-repeated batches pays
        e_tot_local = batch.n_segments
        # (three fresh batches, the fastest counts: a first large allocation after the timed loop was
        # seen to add 50 ms to a single measurement on some boxes)
        t_plan_warm = t_fresh_fwd = float("inf")
        warm_runs = []
        for _ in range(3):
            fresh = HitGraphBatch.from_graphs(graphs).to(dev)
            # (building the host arrays of 256 graphs idles the GPU for ~0.3 s and its clocks fall; a stream of
            # never-repeated batches keeps it busy - twenty forwards of the resident batch bring the clocks back)
            for _w in range(20):
                model(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh.build_plan(D, limits)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            model(fresh)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            warm_runs.append((t1 - t0) * 1e3)
            if t2 - t0 < t_plan_warm + t_fresh_fwd:
                t_plan_warm, t_fresh_fwd = t1 - t0, t2 - t1
        # where a batch is put together: on the host (from_graphs + upload) or on the device from a dataset resident in
        # HBM (batcher.GraphStore) - outside every timed region above, on the record beside them
        assembly = None
        if world == 1:
            from gnn_fpga_amd.batcher import GraphStore
            t0 = time.perf_counter()
            hb = HitGraphBatch.from_graphs(graphs)
            t1 = time.perf_counter()
            hb = hb.to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            del hb
            store = GraphStore(graphs, device=dev)
            t_st = float("inf")
            for _ in range(3):
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                sb, _y = store.batch(0, len(graphs), "flat")
                torch.cuda.synchronize()
                t_st = min(t_st, time.perf_counter() - t3)
            assembly = {"host_from_graphs_ms": (t1 - t0) * 1e3, "upload_ms": (t2 - t1) * 1e3,
                        "graph_store_on_device_ms": t_st * 1e3,
                        "note": "one batch of the workload's graphs: HitGraphBatch.from_graphs (numpy) + .to(device), "
                                "against GraphStore.batch (the dataset resident in HBM, slices + one offset add there)"}
            del store, sb
        # the same never-seen batch on the model's default first-forward route (no plan: segment lists by
        # gnn_csr_build + the per-module kernels)
        t_first = float("inf")
        for _ in range(3):
            unseen = HitGraphBatch.from_graphs(graphs).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(unseen)
            torch.cuda.synchronize()
            t_first = min(t_first, time.perf_counter() - t0)
            del unseen
        pruned = None
        if args.workload == "c3" and world == 1 and not args.no_pruned:
            # the same model with masks that kill half of every layer's units (whole
            # rows / columns, the pattern of the reference's pruned model): compact_dead_units hands
            # the hidden_dim-4 kernels a narrower network that computes the same function
            C = F + D
            me = [torch.ones(D, 2 * C), torch.ones(1, D)]
            mn = [torch.ones(D, 3 * C), torch.ones(D, D)]
            for n, i in enumerate((1, 3, 4, 6)):
                (me[0].__setitem__((i, slice(None)), 0) if n % 2 == 0 else me[1].__setitem__((0, i), 0))
            for n, i in enumerate((0, 2, 5, 7)):
                (mn[0].__setitem__((i, slice(None)), 0) if n % 2 == 0 else mn[1].__setitem__((slice(None), i), 0))
            for k in (2, 3, 5, 6):
                for blk, msk in ((2, me[0]), (3, mn[0])):
                    for b in range(blk):
                        msk[:, b * C + k] = 0
            torch.manual_seed(0)
            pm = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T, masks_e=me, masks_n=mn).to(dev).eval()
            pm.use_events = False
            info = pm.pruned_info()
            ps = max(args.steps // 4, 5)
            times = {}
            for on in (False, True):
                pm.prune_dead_units = on
                pm.invalidate()
                for _ in range(3):
                    pm(fresh)
                times[on] = time_steps(lambda: pm(fresh), ps, sync_all) / ps
            pruned = {"masks": "4 of 8 edge hidden units, 4 of 8 node hidden units and 4 of 8 hit "
                               "features dead (whole rows / columns masked)",
                      "kernels_hidden_dim": info and info["hidden_dim"],
                      "ms_per_step_full_width": times[False] * 1e3, "ms_per_step": times[True] * 1e3,
                      "speedup": times[False] / times[True], "value": e_tot_local / times[True]}
            # the reference's OWN pruned model (gnn/MPNN_Seg_ACTS_maskedlinear.ipynb cell 34: 2 of 8 edge hidden units
            # dead, nothing else): no narrower width exists for it - on the record as such
            me2 = [torch.ones(D, 2 * C), torch.ones(1, D)]
            me2[0][1, :] = 0
            me2[0][6, :] = 0
            torch.manual_seed(0)
            pe = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T, masks_e=me2,
                                   masks_n=[torch.ones(D, 3 * C), torch.ones(D, D)]).to(dev).eval()
            pe.use_events = False
            for _ in range(3):
                pe(fresh)
            t_eo = time_steps(lambda: pe(fresh), ps, sync_all) / ps
            einfo = pe.pruned_info()
            pruned["edge_only"] = {"masks": "2 of 8 edge hidden units dead (the reference's pruned model)",
                                   "kernels_hidden_dim": (einfo and einfo["hidden_dim"]) or D,
                                   "ms_per_step": t_eo * 1e3,
                                   "note": "no specialisation: six live units still occupy a hit's four lanes"}
        del fresh
    if world > 1:
        tmax = torch.tensor([elapsed, exact or 0.0], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax[0].item())
        exact = float(tmax[1].item()) or None

    train, train_capture = (None, None) if args.no_train else train_c4(dev, rank, world, rehearse)
    if train_capture is not None and world == 1:
        train_capture()
    train3 = train5 = None
    if not args.no_train and world == 1 and args.workload == "c3" and len(graphs) >= 32:
        train3 = train_c3(dev, graphs)
    if not args.no_train and world == 1 and args.workload == "c5":
        train5 = train_c3(dev, graphs, steps=15, warmup=4, hidden_dim=D, n_iters=T, n_graphs=1)

    c5 = single = None
    if world == 1 and args.workload == "c3" and not args.no_c5 and not args.graph:
        c5 = c5_record(dev, args.steps, args.pmc_traffic)
    if world == 1 and not args.graph:
        with torch.no_grad():
            single = fresh_single_graph(dev, model, graphs[0], D)

    if rank == 0:
        per = {}
        for name, ms in seq:
            per.setdefault(name, []).append(ms)
        tot = {k: sum(v) for k, v in per.items()}
        dom = max(tot, key=tot.get)
        avg_ms = {k: sum(v) / len(v) for k, v in per.items()}
        n_tot, e_tot = batch.n_hits, batch.n_segments
        alg = algorithmic(n_tot, e_tot, F, D, T, w=2 if bf16 else 4)
        ab, af = alg["bytes"], alg["flops"]
        # algorithmic bytes of the dominant kernel's launches in one step; when the input network
        # is fused into the first iteration launch (no k_input4 launch), its bytes ride along
        n_dom = len(per[dom])
        ab_dom_step, af_dom_step = n_dom * ab[dom], n_dom * af[dom]
        if dom == "k_iter2" and "k_input4" not in per:
            ab_dom_step += ab["k_input4"]
            af_dom_step += af["k_input4"]
        ab_dom, af_dom = ab_dom_step / n_dom, af_dom_step / n_dom          # average per launch
        t_dom = avg_ms[dom] * 1e-3
        gbs = ab_dom / t_dom / 1e9
        tfs = af_dom / t_dom / 1e12
        ms_step = elapsed / args.steps * 1e3
        traffic = traffic_source = None
        sec = pmc_section(args.pmc_traffic, args.workload if args.workload == "c3" else
                          "c5_" + ("bf16" if bf16 else "f32"))
        if sec and G == wl["G"]:
            # the dominant kernel has template variants (first / middle / last iteration move
            # different amounts): launch-weighted mean over the profiled run
            traffic = kernel_traffic(sec, dom)
            if traffic:
                traffic_source = ("%s (%s): rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE passes of this "
                                  "command, committed - not measured in this run"
                                  % (os.path.relpath(args.pmc_traffic, REPO), sec.get("source", "?")))
        sum_k = sum(ms for _, ms in seq)
        dom_pos = per[dom]
        roof = {"kernel": dom, "algorithmic_bytes_per_launch": ab_dom,
                "algorithmic_flops_per_launch": af_dom, "avg_launch_ms": avg_ms[dom],
                # flat scalars (nested objects do not survive the driver's parse): the dominant
                # kernel by launch position, everything else in one number, and the cross-check
                "launches_per_step": n_dom,
                "launch_ms_first": dom_pos[0], "launch_ms_middle": dom_pos[len(dom_pos) // 2],
                "launch_ms_last": dom_pos[-1],
                "other_kernels_ms": sum_k - sum(dom_pos),
                "sum_kernel_ms": sum_k, "ms_per_step": ms_step,
                "consistent": bool(sum_k <= 1.05 * ms_step),
                "timed_regions_ms_per_step": [t / args.steps * 1e3 for t in timed_regions],
                "timing": "HIP events on the launch stream, %d-step pass after the timed loop, first third "
                          "dropped, median per launch position" % min(max(3 * args.steps, 30), 600),
                "traffic": traffic, "traffic_source": traffic_source,
                "kernel_ms": {k: round(v, 4) for k, v in avg_ms.items()},
                "launch_sequence_ms": [[k, round(v, 4)] for k, v in seq],
                "forward_algorithmic_GBps": ab["forward"] / (ms_step * 1e-3) / 1e9,
                "forward_frac": ab["forward"] / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS}
        # (c5 too: the kernels execute the per-hit P/Q form, E/N = 10x fewer multiply-adds than the
        # reference's per-segment contraction, so its nominal MFMA figure bounds nothing - the
        # bytes do; the algorithmic flop rate stays in the record for reference)
        roof = dict({"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": gbs / HBM_PEAK_GBS}, **roof)
        if args.workload == "c5":
            roof["algorithmic_TFLOPs"] = tfs
            if sec:
                roof["valu_busy"] = sec.get("valu_busy", {}).get(dom)
        out = headline(args, wl, world, batch, plan, elapsed, bf16, G, dumped)
        out.update({
            "roofline": roof,
            "plan_ms": {"cold": t_plan * 1e3, "warm": t_plan_warm * 1e3, "warm_runs": warm_runs,
                        "builder": type(plan).__name__,
                        "stage1": ("graph-local (one workgroup per graph / per tile, LDS tables; neighbour lists %s)"
                                   % ("per tile in LDS" if getattr(plan, "list_mode", 0) else "by scattered pairs + a sort per list")
                                   if getattr(plan, "graph_local", False) else "global (device-wide sweeps and radix sorts)"),
                        "fresh_batch_forward_ms": t_fresh_fwd * 1e3},
            "value_fresh_batch": e_tot / t_first,
            "fresh_batch_ms": t_first * 1e3,
            "value_fresh_batch_note": "one forward on a never-seen batch on the default route for it (no plan: "
                                      "gnn_csr_build + per-module kernels), synchronised wall clock, best of 3",
            "value_incl_plan": e_tot / (t_plan_warm + t_fresh_fwd),
            "value_incl_plan_note": "one forward on a never-seen batch: warm plan build + first forward; "
                                    "`value` replays one resident batch (plan amortised)",
        })
        if assembly is not None:
            out["batch_assembly_ms"] = assembly
        if exact is not None:
            out["value_exact_exp"] = world * e_tot / exact
            out["ms_per_step_exact_exp"] = exact * 1e3
        if single is not None:
            out["fresh_single_graph_ms"] = single["ms"]
            out["fresh_single_graph"] = single
        if c5 is not None:
            out["c5"] = c5
        if other is not None:
            out["other_dtype"] = {"dtype": "f32" if bf16 else "bf16", "ms_per_step": other * 1e3,
                                  "value": e_tot / other}
        if pruned is not None:
            out["pruned"] = pruned
        if train is not None:
            out["train_c4"] = train
        if train3 is not None:
            out["train_c3"] = train3
        if train5 is not None:
            out["train_c5"] = train5
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(model, graphs[0], wl)
    if train_capture is not None and world > 1:
        # LAST, behind a watchdog: a capture with a collective inside cannot be rehearsed on a one-GPU
        # box; if it does not come back, rank 0 still prints the line (eager numbers) and every rank
        # leaves with code 0
        import threading

        def bail():
            if rank == 0:
                out["train_c4"]["hip_graph"] = "capture / replay did not finish within 180 s - eager numbers only"
                print(json.dumps(out), flush=True)
            os._exit(0)

        timer = threading.Timer(180.0, bail)
        timer.daemon = True
        timer.start()
        train_capture()
        timer.cancel()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c3")
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16", help="c5 only")
    ap.add_argument("--graphs", type=int, default=0, help="graphs per launch per GPU (default: 256 c3, 8 c5)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: roofline, exact-exp and other-dtype rates, plan and "
                         "fresh-batch costs, c5, pruned, training steps, CPU baseline (the --no-* options "
                         "below trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the scores of the last timed step to DIR/scores.npy (float32, a fixed sample "
                         "beyond 2^23 segments)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-train", action="store_true", help="skip the train_c4 sub-record")
    ap.add_argument("--no-pruned", action="store_true", help="skip the pruned-model sub-record (c3, N=1)")
    ap.add_argument("--no-c5", action="store_true", help="skip the c5 sub-record (c3, N=1)")
    ap.add_argument("--dry-run", action="store_true",
                    help="start the ranks, rendezvous over gloo, print {dry_run, ranks} and leave (no GPU)")
    ap.add_argument("--graph", action="store_true",
                    help="experiment: replay the forward from a captured HIP graph")
    ap.add_argument("--global-gather", action="store_true",
                    help="experiment: disable the LDS windows (gather records from global memory)")
    ap.add_argument("--pmc-traffic", default=os.path.join(REPO, "profiles", "pmc_traffic.json"),
                    help="per-kernel HBM bytes per launch from separate rocprofv3 --pmc passes of "
                         "this same command (FETCH_SIZE x2 + WRITE_SIZE, MI355X_MICROARCH.md), "
                         "written by tools/profile_bench.sh; `traffic` is null without it")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    world = os.environ.get("WORLD_SIZE")
    if world is None and args.gpus > 1:
        sys.exit(launch_ranks(args))
    if int(world or 1) != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%s: launch with torch.distributed.run "
                         "--nproc-per-node %d, or unset WORLD_SIZE and bench.py starts the ranks itself"
                         % (args.gpus, world, args.gpus))
    run(args)


if __name__ == "__main__":
    main()
