#!/usr/bin/env python
"""Headline benchmark: NN evaluations/sec of the crazyhouse RISEv2-19 path at batch 256 (+ MCTS nodes/sec and the rest with --full).

Contract: `python bench.py --gpus N --steps K --warmup W` (N>1 is launched by torch.distributed.run, one rank per
GPU).  One step = one pass of the hot path over one batch of synthetic positions already resident in HBM:
input planes -> RISEv2 19-block forward -> policy softmax + value (what NeuralNetAPI::predict computes between its
H2D and D2H copies, engine/src/nn/tensorrtapi.cpp:195-237).  Rank 0 prints ONE JSON line.

Such a plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line, nothing else.  --full adds
everything else the benchmark measures after the timed region: the other precision modes and batch sizes, the PCIe-inclusive
rates, the per-kernel roofline with its live PMC passes, the search / game / drop-in legs and the CPU baseline.

The metric follows CrazyAra::inference (engine/src/uci/crazyara.cpp:156-181): evals/s = steps * batchSize / elapsed.
Multi-GPU = independent replicas: no data-path collective, only the final reduction of the
timing/throughput scalars over RCCL.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

BATCH = 256
N_BLOCKS = 19
PEAK_F16_TFLOPS = 2500.0      # MI355X dense f16/bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5000.0      # dense fp8 MFMA peak (v_mfma_f32_32x32x64_f8f6f4 measures 4.41 PFLOP/s at the 2.10 GHz it settles at)
PEAK_HBM_GBS = 8000.0
# op name (mi_net_time_ops) -> substring of the kernel symbol ("tower_x3_" matches the two-role and the symmetric kernel)
KERNEL_SYMBOL = {"fused_block": "block_kernel", "block_x3": "block_x3_kernel", "tower_x3": "tower_x3_", "tower_p8": "tower_p8_kernel"}


def synthetic_planes(batch, channels, seed):
    """Board-like planes: ~88 % exact zeros, sparse ones, a few fractional constant planes."""
    rng = np.random.default_rng(seed)
    x = (rng.random((batch, channels, 8, 8)) < 0.10).astype(np.float32)
    for b in range(batch):
        for c in rng.choice(channels, size=max(2, channels // 8), replace=False):
            x[b, c] = rng.choice([0.0, 1.0, 0.25, 1.0 / 32, 3.0 / 8])
    return torch.from_numpy(x)


def committed_pmc_traffic(kernel: str):
    """roofline.traffic: fabric-side bytes per launch of the dominant kernel from the PMC passes committed under profiles/
    (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in their own runs, scripts/gpu_round.sh; FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for 16-byte-per-lane streaming reads on gfx950; both counters are KiB).  PMC passes cannot run
    inside the timed process, so this is the newest committed measurement of the same workload, or null."""
    import glob
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    symbol = KERNEL_SYMBOL.get(kernel, f"{kernel}_kernel")

    def counter(path, name):
        if not os.path.exists(path):
            return None
        block = False
        for line in open(path):
            if line.startswith("=="):
                block = symbol in line
            elif block and line.split()[:1] == [name]:
                m = re.search(r"mean\s+([0-9.]+)", line)
                return float(m.group(1)) if m else None
        return None
    # newest committed pass (by round directory, then set letter) that holds this kernel
    for f1 in sorted(glob.glob(os.path.join(root, "r*", "*_pmc_*tcc1.txt")), reverse=True):
        f2 = f1.replace("tcc1.txt", "tcc2.txt")
        fetch, write = counter(f1, "FETCH_SIZE"), counter(f2, "WRITE_SIZE")
        if fetch is not None and write is not None:
            return {"traffic": round((2.0 * fetch + write) * 1024.0), "traffic_unit": "bytes per launch (2 x FETCH_SIZE + WRITE_SIZE)",
                    "traffic_source": os.path.relpath(f1, os.path.dirname(root))}
    return {"traffic": None}


def live_pmc_traffic(kernel: str, blocks: int, batch: int, precision: str, timeout_s: int = 150):
    """roofline.traffic measured NOW, on this box: two `rocprofv3 --pmc` passes (counters only, no trace domains) of
    scripts/prof_forward.py -- the same network, batch and device-resident forward as the timed region -- in child processes, summed
    per dispatch of the dominant kernel: 2 x FETCH_SIZE + WRITE_SIZE (KiB counters; FETCH_SIZE doubled as MI355X_MICROARCH.md
    prescribes for 16-byte-per-lane streaming reads on gfx950).  Returns None when rocprofv3 is missing, times out or reports nothing
    (the caller then falls back to the newest committed pass and says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None:
        return None
    out = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for counters in (["FETCH_SIZE", "TCC_HIT_sum"], ["WRITE_SIZE", "TCC_MISS_sum"]):
        d = tempfile.mkdtemp(prefix="cra_pmc_", dir="/tmp")
        cmd = [rocprof, "--pmc", *counters, "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.join(ROOT, "scripts", "prof_forward.py"), str(blocks), str(batch), precision, "3"]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout_s)
        except (subprocess.TimeoutExpired, OSError):
            shutil.rmtree(d, ignore_errors=True)
            return None
        if r.returncode != 0:
            shutil.rmtree(d, ignore_errors=True)
            return None
        vals = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if KERNEL_SYMBOL.get(kernel, f"{kernel}_kernel") in row["Kernel_Name"]:
                    vals.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        shutil.rmtree(d, ignore_errors=True)
        for c in counters:
            if c not in vals:
                return None
            out[c] = sum(vals[c]) / len(vals[c])
    return {"traffic": round((2.0 * out["FETCH_SIZE"] + out["WRITE_SIZE"]) * 1024.0),
            "traffic_unit": "bytes per launch (2 x FETCH_SIZE + WRITE_SIZE)",
            "traffic_source": "live: rocprofv3 --pmc passes of scripts/prof_forward.py run by this bench.py on this box",
            "pmc": {"FETCH_SIZE_KiB": round(out["FETCH_SIZE"], 1), "WRITE_SIZE_KiB": round(out["WRITE_SIZE"], 1),
                    "TCC_HIT_sum": round(out["TCC_HIT_sum"]), "TCC_MISS_sum": round(out["TCC_MISS_sum"]),
                    "l2_to_cu_bytes_per_launch": round(out["TCC_HIT_sum"] * 128.0)}}


def cpu_model_string():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, sd, x, budget_s=20.0):
    """Reference CPU path timed beside the GPU: the reference's OWN PyTorch module when /root/reference is
    importable (this container; kind "reference"), else the oracle restatement of it (the GPU box; kind "port": the same torch ops in the
    same order, pinned to the reference module by tests/golden/nn_*.npz) -- fp32, eval, no_grad, softmax included, on the host cores.
    As CrazyAra::inference does (crazyara.cpp:156-181) the loop is warmed first (its 100 iterations, bounded here to ~3 s), then timed
    over >= 5 samples of whole batches; `value` = the MEDIAN sample, the quartiles and the CPU's model string beside it, so that two
    runs on one box can be told from two boxes."""
    from crazyara_amd import replicas
    from oracle import rise_oracle as ro
    # measured on the MI355X host (256 logical CPUs): torch CPU inference peaks at 16 threads (8: 183, 16: 474, 32: 374,
    # 64: 198, 128: 80 evals/s on this model) -- more threads oversubscribe the 8x8 convolutions
    cores = min(16, replicas.available_cpus())
    torch.set_num_threads(cores)
    kind, fn = "port", (lambda xb: ro.predict(cfg, sd, xb))
    if os.path.isdir("/root/reference/DeepCrazyhouse"):
        try:
            from oracle import make_golden
            model = make_golden.reference_model(make_golden.import_reference(), cfg)
            model.load_state_dict(sd)
            model.eval()

            def fn(xb, model=model):
                with torch.no_grad():
                    out = model(xb)
                    return out[0], torch.softmax(out[1], 1)
            kind = "reference"
        except Exception:  # noqa: BLE001 -- the reference would not import: the port is the baseline, and says so
            kind = "port"
    t0, n_warm = time.perf_counter(), 0
    while n_warm < 100 and time.perf_counter() - t0 < 3.0:
        fn(x[:64])
        n_warm += 1
    rates, n_total, el_total = [], 0, 0.0
    per_sample = (budget_s - 3.0) / 5.0
    while len(rates) < 5 or (el_total < budget_s - 3.0 and len(rates) < 9):
        n, t0 = 0, time.perf_counter()
        while True:
            fn(x)
            n += x.shape[0]
            el = time.perf_counter() - t0
            if el > per_sample or n >= 8 * x.shape[0]:
                break
        rates.append(n / el)
        n_total += n
        el_total += el
    q1, med, q3 = (float(v) for v in np.percentile(rates, [25, 50, 75]))
    out = {"value": round(med, 1), "unit": "evals/s", "cores": cores, "kind": kind,
           "value_q1": round(q1, 1), "value_q3": round(q3, 1), "iqr_over_median": round((q3 - q1) / med, 4), "n_samples": len(rates),
           "samples_evals_per_sec": [round(r, 1) for r in rates], "cpu_model": cpu_model_string(), "warmup_iterations": n_warm,
           "sample": f"{len(rates)} samples, {n_total} positions (batches of {x.shape[0]}) of the same synthetic workload, "
                     + ("the reference RiseV3 module (rise_mobile_v3.py)" if kind == "reference" else "oracle/rise_oracle.predict (torch restatement of RiseV3)")
                     + f", fp32, {cores} threads, {el_total:.1f} s; value = median"}
    out.update(cpu_baseline_mcts(cfg, sd, cores))
    out.update(cpu_baseline_reference_search(cores))
    return out


def cpu_baseline_reference_search(cores):
    """BASELINE config 1 as the reference runs it without a GPU: the reference's OWN search code (MCTSAgent / SearchThread / Node ...,
    compiled unmodified into oracle/_ref/libcrazyara_ref.so) on the crazyhouse start position, RISEv2-7, batch 8, 800 simulations,
    with the CPU net (oracle port of the reference PyTorch module) behind its NeuralNetAPI.  kind = "reference" for the search code."""
    from crazyara_amd import env, rise_config, search
    from oracle import ref_mcts, rise_oracle as ro
    try:
        ref_mcts.load()
    except Exception as e:  # noqa: BLE001 -- the prebuilt file did not travel: report it, never fail the bench
        return {"config1_reference_search": {"skipped": f"oracle/_ref/libcrazyara_ref.so not loadable: {e}"}}
    cfg = rise_config.rise_v2_config(7, 34, 81)
    sd = rise_config.make_state_dict(cfg, seed=31, stress=True)
    layout = env._capi.load().mi_planes_layout(0, 1)
    evals = [0]

    def eval_descs(descs):
        planes = env.planes_from_descs_host(b"".join(descs), len(descs), layout, True)
        v, p, _ = ro.predict(cfg, sd, torch.from_numpy(planes))
        evals[0] += len(descs)
        return v.numpy(), p.numpy()

    st = search.default_settings(mode=0, version_major=1, batch_size=8)
    agent = ref_mcts.RefAgent(st, eval_descs, cfg.nb_policy)
    agent.set_position("", False, "crazyhouse")
    t0 = time.perf_counter()
    agent.go(simulations=800)
    el = time.perf_counter() - t0
    info = agent.root_info()
    agent.close()
    return {"config1_reference_search": {
        "mcts_nodes_per_sec": round((info["node_count"]) / el, 1), "nn_evals": evals[0], "seconds": round(el, 2), "cores": cores,
        "kind": "reference",
        "sample": "the reference's MCTSAgent (one SearchThread, batch 8) on the crazyhouse start position, 800 simulations, RISEv2-7 "
                  "evaluated by the oracle CPU net behind the callback NeuralNetAPI"}}


def cpu_baseline_mcts(cfg, sd, cores, trees=16, quota=16, simulations=48):
    """Metric 2 on the CPU path: the SAME C++ leaf collector with the CPU net plugged in behind the evaluator
    boundary -- descriptors -> host plane builder -> oracle network.  Bounded: 16 trees x 48 simulations, one lane, batch 256."""
    from crazyara_amd import env, openings, search
    from oracle import rise_oracle as ro
    st = search.default_settings(mode=0, version_major=1, batch_size=quota)
    layout = env._capi.load().mi_planes_layout(0, 1)

    def eval_descs(descs):
        planes = env.planes_from_descs_host(b"".join(descs), len(descs), layout, True)
        v, p, _ = ro.predict(cfg, sd, torch.from_numpy(planes))
        return v.numpy(), p.numpy()

    pool = search.SearchPool(st, eval_fn=eval_descs, fn_batch=trees * quota, fn_nb_policy=cfg.nb_policy)
    fens = openings.position_fens("crazyhouse")
    for i in range(trees):
        pool.add_position(fens[(i * 7) % len(fens)], False, "crazyhouse")
    stt = pool.run(simulations=simulations, threads=min(cores, trees))
    pool.close()
    return {"mcts_nodes_per_sec": round(stt.nodes / stt.seconds, 1), "mcts_nn_evals_per_sec": round(stt.nn_evals / stt.seconds, 1),
            "mcts_sample": f"{trees} trees x {simulations} simulations of the opening set, C++ leaf collector + oracle CPU net "
                           f"behind the evaluator callback, {stt.seconds:.1f} s"}


def dropin_reference_search(model_dir, device, batch, precisions=("float16x3", "float16"), threads_list=(1, 2, 4, 8)):
    """The number a CrazyAra maintainer gets after the three edits of INTEGRATION.md: the reference's OWN MCTSAgent + SearchThreads
    (compiled from /root/reference into oracle/_ref/libcrazyara_ref_hip_release.so with the reference's Release flags, searchthread.cpp:403-416) on HipAPI nets
    (integration/hipapi.h -> mi_net_predict), `Threads` = 1 / 2 / 4 / 8, Batch_Size 256.  Two workloads: BASELINE config 2 (crazyhouse
    openings, 1600 simulations per go) and CrazyAra::benchmark's 15 positions (3200 simulations per go, crazyara.cpp:287-330).
    A MEASUREMENT leg like cpu_baseline (kind "reference"): the product path never runs this code."""
    from crazyara_amd import openings, search
    from oracle import ref_mcts
    try:
        ref_mcts.load_hip(release=True)
    except Exception as e:  # noqa: BLE001 -- the prebuilt file did not travel: report it, never fail the bench
        return {"skipped": f"oracle/_ref/libcrazyara_ref_hip_release.so not loadable: {e}"}
    st = search.default_settings(mode=0, version_major=1, batch_size=batch)
    opening_fens = openings.crazyhouse_opening_set()[::7][:10]
    table = openings.benchmark_positions()
    out = {"kind": "reference", "batch_size": batch,
           "workload": "the reference's MCTSAgent / SearchThread (oracle/_ref/libcrazyara_ref_hip_release.so, -O3 -DNDEBUG) on HipAPI nets, RISEv2-19, Batch_Size 256: "
                       "config2 = 10 crazyhouse openings x go simulations 1600; benchmark = the 15 positions of benchmarkpositions.cpp x go "
                       "simulations 3200; nodes = visits - freeVisits at the root (evalinfo.cpp:73-80)"}
    # the same with integration/searchthread_hip.patch applied to the reference's SearchThread (descriptor-fed batches, priors gathered
    # on the GPU; kind "reference+patch", headline mode only): oracle/_ref/libcrazyara_ref_hip_patched_release.so
    runs = [(precision, th, False) for precision in precisions for th in threads_list]
    try:
        ref_mcts.load_hip(release=True, patched=True)
        runs += [(precisions[0], th, True) for th in threads_list]
        out["patched_kind"] = "reference+patch"
    except Exception as e:  # noqa: BLE001
        out["patched_skipped"] = f"oracle/_ref/libcrazyara_ref_hip_patched_release.so not loadable: {e}"
    for precision, th, patched in runs:
        if True:
            agent = ref_mcts.RefAgent(st, hip_model_dir=model_dir, device_id=device, precision=precision, threads=th, release=True, patched=patched)
            agent.set_position(opening_fens[0], False, "crazyhouse")
            agent.go(simulations=400)                                      # warm-up: kernels loaded, pinned buffers touched
            rates = {}
            for name, fens, sims in (("config2", opening_fens, 1600), ("benchmark", [t["fen"] for t in table], 3200)):
                nodes, secs = 0, 0.0
                for f in fens:
                    agent.set_position(f, False, "crazyhouse")
                    t0 = time.perf_counter()
                    agent.go(simulations=sims)
                    secs += time.perf_counter() - t0
                    nodes += agent.root_info()["node_count"]
                rates[name] = round(nodes / secs, 1)
            agent.close()
            out[f"{precision}{'_patched' if patched else ''}_threads_{th}"] = {"config2_mcts_nodes_per_sec": rates["config2"],
                                                                                 "benchmark_mcts_nodes_per_sec": rates["benchmark"]}
    return out


def config_search_legs(args, device, threads):
    """nodes/sec of the BASELINE.json configurations that are not the headline, each with its own network family, batch size,
    simulation limit and position set: config 1 = one position, one tree, batch 8 -- a single UCI `go`."""
    from crazyara_amd import netfile, openings, rise_config, search, searchbench
    from crazyara_amd.neuralnetapi import HipAPI
    out = {}

    other = getattr(args, "search_precision_other", None)
    if other == args.precision:
        other = None

    def nets_for(cfg, version, batch, lanes, seed, precision=None):
        sd = rise_config.make_state_dict(cfg, seed=seed, stress=True)
        d = tempfile.mkdtemp(prefix="cra_bench_cfg_")
        netfile.export_rise(os.path.join(d, f"{cfg.name}-v{version}.cranet"), cfg, sd, input_version=version)
        return [HipAPI(device, batch, d, precision or args.precision) for _ in range(lanes)]

    def leg(name, workload, cfg, version, mode, batch, lanes, quota, sims, positions, trees, shared=0, also_other=False):
        """The leg with nets of the line's precision mode; also_other: once more (one repeat) with nets of --search-precision-other,
        reported inside the same entry as mcts_nodes_per_sec_<mode>."""
        st = search.default_settings(mode=mode, version_major=int(version.split(".")[0]), batch_size=quota)
        leg_threads = min(threads, shared * lanes) if shared else min(threads, max(1, trees // max(1, lanes)))
        for prec in [args.precision] + ([other] if also_other and other else []):
            nets = nets_for(cfg, version, batch, lanes, seed=31, precision=prec)
            r = searchbench.timed_search_leg(st, nets, positions, trees, sims, max(1, leg_threads), min_seconds=args.search_seconds,
                                             repeats=args.search_repeats if prec == args.precision else 1, shared_collectors=shared)
            for n in nets:
                n.close()
            if prec != args.precision:
                out[name][f"mcts_nodes_per_sec_{prec}"] = r["mcts_nodes_per_sec"]
                continue
            r.pop("_median_totals")
            r.pop("_spread")
            r["workload"] = workload
            r["per_tree_quota"] = quota
            r["precision"] = prec
            out[name] = r

    cz = [(f, False, "crazyhouse") for f in openings.crazyhouse_opening_set()]
    # config 1: the crazyhouse start position (then the rest of the opening set, one position per round), ONE tree, batch 8
    leg("config1", "crazyhouse start position + opening set one at a time, RISEv2-7, batch 8, 800 simulations, ONE tree (a single UCI go)",
        rise_config.rise_v2_config(7, 34, 81), "1.0", 0, 8, 1, 8, 800, cz, 1, also_other=True)
    leg("config1_two_search_threads", "the same with the reference's default Threads = 2: two collectors (one per lane, batch 8 each) "
        "share the one tree", rise_config.rise_v2_config(7, 34, 81), "1.0", 0, 8, 2, 8, 800, cz, 1, shared=1, also_other=True)
    # `Threads` is a UCI option (optionsuci.cpp:182): a batch of 8 occupies 8 of the 256 CUs, so more collectors on the one tree put more
    # batches of 8 on the GPU at the same time
    leg("config1_four_search_threads", "the same with Threads = 4: four collectors (one per lane, batch 8 each) share the one tree",
        rise_config.rise_v2_config(7, 34, 81), "1.0", 0, 8, 4, 8, 800, cz, 1, shared=1)
    leg("config1_eight_search_threads", "the same with Threads = 8", rise_config.rise_v2_config(7, 34, 81), "1.0", 0, 8, 8, 8, 800, cz, 1, shared=1)
    # the same eight collectors of 8 leaves each arranged as the pool prefers them: two lanes, four collectors per lane collected in
    # parallel on four threads, a lane's batch = their 32 leaves (a lane is driven by one thread: eight lanes of one collector serialise
    # their collection on it)
    leg("config1_eight_collectors_two_lanes", "ONE tree, 8 collectors x 8 leaves as 2 lanes x 4 collectors (batch 32 per lane), 800 simulations",
        rise_config.rise_v2_config(7, 34, 81), "1.0", 0, 32, 2, 8, 800, cz, 1, shared=4, also_other=True)
    # the single-position reading of config 2: one tree fills the whole batch of 256 by itself
    leg("config2_one_tree", "one crazyhouse position at a time, RISEv2-19, batch 256 collected from ONE tree by one collector, "
        "1600 simulations", rise_config.rise_v2_config(19, 34, 81), "1.0", 0, 256, 1, 256, 1600, cz, 1)
    leg("config2_one_tree_shared", "one crazyhouse position at a time, RISEv2-19, 2 lanes x batch 256, ONE tree shared by 8 collectors "
        "per lane (32 leaves each) under per-node locks, 1600 simulations", rise_config.rise_v2_config(19, 34, 81), "1.0", 0, 256, 2, 32,
        1600, cz, 1, shared=8, also_other=True)
    leg("config2_one_tree_three_lanes", "the same tree with a third lane (3 x 256 leaves in flight, 8 collectors per lane)",
        rise_config.rise_v2_config(19, 34, 81), "1.0", 0, 256, 3, 32, 1600, cz, 1, shared=8)
    leg("config2_one_tree_shared_6400", "the same with 6400 simulations per go (a longer think)",
        rise_config.rise_v2_config(19, 34, 81), "1.0", 0, 256, 2, 32, 6400, cz, 1, shared=8)
    # the lane shape that serves ONE tree best (profiles/r05/f_one_tree_sweep_*: 2 / 3 lanes x 256, 4-6 x 128, 8-12 x 64, 16 x 32 at 1600
    # and 6400 simulations): a third batch in flight pays once the tree is wide enough to fill it
    leg("config2_one_tree_three_lanes_6400", "ONE tree, 3 lanes x 256, 8 collectors per lane, 6400 simulations per go",
        rise_config.rise_v2_config(19, 34, 81), "1.0", 0, 256, 3, 32, 6400, cz, 1, shared=8)
    # CrazyAra::benchmark on its own position table (one tree, one go per position)
    nets = nets_for(rise_config.rise_v2_config(19, 34, 81), "1.0", 256, 2, seed=31)
    st_b = search.default_settings(mode=0, version_major=1, batch_size=32)
    out["benchmark_positions"] = searchbench.benchmark_positions_leg(st_b, nets, 3200, min(threads, 16), shared_collectors=8)
    out["benchmark_positions"]["precision"] = args.precision
    for n in nets:
        n.close()
    if other:
        nets = nets_for(rise_config.rise_v2_config(19, 34, 81), "1.0", 256, 2, seed=31, precision=other)
        out["benchmark_positions"][f"mcts_nodes_per_sec_{other}"] = searchbench.benchmark_positions_leg(
            st_b, nets, 3200, min(threads, 16), shared_collectors=8)["mcts_nodes_per_sec"]
        for n in nets:
            n.close()
    chess = [(f, False, "chess") for f in openings.position_fens("chess")]
    leg("config3", "standard chess calibration-game positions, RISEv3.3, batch 512, 3200 simulations, 2 lanes x 32 trees",
        rise_config.rise_v33_config(52, 76, False), "3.0", 1, 512, 2, 16, 3200, chess, 64, also_other=True)
    from crazyara_amd import _capi
    lib = _capi.load()
    c960 = [(lib.mi_chess960_start_fen((i * 97 + 13) % 960).decode(), True, "chess") for i in range(96)]
    leg("config4_one_gpu", "chess960 start positions (Scharnagl numbers), 8 concurrent games' trees, RISEv3.3, batch 256, 1600 simulations "
        "(the one-GPU slice of config 4)", rise_config.rise_v33_config(52, 76, False), "3.0", 1, 256, 2, 64, 1600, c960, 8, also_other=True)
    mixed = []
    a, b = searchbench.variant_positions("3check"), searchbench.variant_positions("kingofthehill")
    for i in range(max(len(a), len(b))):
        mixed.append(a[i % len(a)])
        mixed.append(b[i % len(b)])
    leg("config5_one_gpu", "3check + king-of-the-hill positions alternating, lichess tables (80-channel planes, 5376 policy), RISEv2-13, "
        "batch 1024, 1600 simulations, 2 lanes x 64 trees (the one-GPU slice of config 5)",
        rise_config.rise_v2_config(13, 80, 84), "3.0", 2, 1024, 2, 16, 1600, mixed, 128, also_other=True)
    return out


def config_game_legs(args, device, threads, rank=0, world=1, selfplay_games=16, arena_games=128, other_mode=True):
    """BASELINE configs 4 and 5 as GAMES: chess960 self-play and a 3check / king-of-the-hill arena between two nets, played by the
    library's native game loops (csrc/rl/selfplay.cpp).  games/min + the nodes/sec of the searches inside.  One GPU: their one-GPU
    slices.  world > 1: the games are SHARDED over the ranks (replicas.shard_items: game g -> rank g % world; this rank plays its
    share from its own start positions); the caller reduces {games, moves, nodes} (SUM) and seconds (MAX) over the ranks."""
    from crazyara_amd import _capi, netfile, replicas, rise_config, search, searchbench, selfplay
    from crazyara_amd.neuralnetapi import HipAPI
    out = {}
    lib = _capi.load()
    my_selfplay = replicas.shard_items(selfplay_games * world, rank, world)        # config 4: `selfplay_games` per GPU (weak scaling)
    my_arena = replicas.shard_items(arena_games * world, rank, world)

    def model_dir(cfg, version, seed, variant):
        sd = rise_config.make_state_dict(cfg, seed=seed, stress=True)
        d = tempfile.mkdtemp(prefix="cra_bench_game_")
        netfile.export_rise(os.path.join(d, f"{cfg.name}-v{version}.cranet"), cfg, sd, input_version=version, variant=variant)
        return d

    def legs(prec):
        res_ = {}
        # config 4: chess960 self-play, 8 concurrent games on this GPU, RISEv3.3, 800 simulations per move, tree reuse, temperature on
        # the first moves (the RL settings' shape; random-init net, so the games are short and mostly drawn by the ply cap)
        d = model_dir(rise_config.rise_v33_config(52, 76, False), "3.0", 41, "chess")
        nets = [HipAPI(device, 256, d, prec) for _ in range(2)]
        st = search.default_settings(mode=1, version_major=3, batch_size=64, seed=5)
        pool = search.SearchPool(st, net_a=nets[0], net_b=nets[1])
        s = selfplay.SelfPlaySettings(variant="chess", is960=True, simulations=800, max_plies=100, mean_init_ply=2.0, init_temperature=0.8,
                                      temperature_moves=8, temperature_decay=0.9, seed=11)
        loop = selfplay.SelfPlay(pool, s, 8, start_fen=lambda i: lib.mi_chess960_start_fen((my_selfplay[i % len(my_selfplay)] * 97 + 13) % 960).decode())
        games = loop.play(len(my_selfplay), threads=min(threads, 8))
        stt = loop.stats
        res_["config4_selfplay_one_gpu"] = {
            "games_per_min": round(len(games) / stt["seconds"] * 60, 1), "games": len(games), "moves": int(stt["moves"]),
            "seconds": round(stt["seconds"], 3), "mcts_nodes_per_sec": round(stt["nodes"] / stt["seconds"], 1),
            "seconds_in_search": round(stt["run_seconds"], 3), "kept_subtrees": int(stt["kept_subtrees"]),
            "workload": "chess960 self-play (native loop), 8 concurrent games, RISEv3.3, batch 256, 800 simulations per move, ply cap 100"}
        loop.close()
        pool.close()
        for n in nets:
            n.close()
        # config 5: arena between two nets on 3check and king-of-the-hill (half of the games each), lichess tables, batch 1024
        cfg5 = rise_config.rise_v2_config(13, 80, 84)
        total = dict(games=0, moves=0, seconds=0.0, nodes=0, wins=0, draws=0, losses=0)
        for variant in ("3check", "kingofthehill"):
            da, db = model_dir(cfg5, "3.0", 42, variant), model_dir(cfg5, "3.0", 43, variant)
            na = [HipAPI(device, 1024, da, prec) for _ in range(2)]
            nb = [HipAPI(device, 1024, db, prec) for _ in range(2)]
            st = search.default_settings(mode=2, version_major=3, batch_size=16, seed=6)
            pa, pb = search.SearchPool(st, net_a=na[0], net_b=na[1]), search.SearchPool(st, net_a=nb[0], net_b=nb[1])
            s = selfplay.SelfPlaySettings(variant=variant, simulations=400, max_plies=80, seed=12)
            starts = [f for f, _, _ in searchbench.variant_positions(variant)]       # one start position per pair of games
            # only the side to move searches, so half of a pool's trees sit out every round: the trees that run share the whole batch
            # (mi_search_set_adaptive_quota) -- 128 concurrent games = 32 running trees per lane x 32 leaves = the batch of 1024
            pa.set_adaptive_quota(32)
            pb.set_adaptive_quota(32)
            arena = selfplay.Arena(pa, pb, s, min(128, len(my_arena)), start_fen=lambda i: starts[my_arena[i % len(my_arena)] % len(starts)])
            res, recs = arena.play(len(my_arena), threads=threads)
            total["games"] += len(recs); total["moves"] += int(arena.stats["moves"]); total["seconds"] += arena.stats["seconds"]
            total["nodes"] += int(arena.stats["nodes"]); total["wins"] += res.wins; total["draws"] += res.draws; total["losses"] += res.losses
            total["run_seconds"] = total.get("run_seconds", 0.0) + arena.stats["run_seconds"]
            total["move_seconds"] = total.get("move_seconds", 0.0) + arena.stats["move_seconds"]
            arena.close()
            pa.close(); pb.close()
            for n in na + nb:
                n.close()
        res_["config5_arena_one_gpu"] = {
            "games_per_min": round(total["games"] / total["seconds"] * 60, 1), "games": total["games"], "moves": total["moves"],
            "seconds": round(total["seconds"], 3), "mcts_nodes_per_sec": round(total["nodes"] / total["seconds"], 1),
            "seconds_in_search": round(total["run_seconds"], 3), "seconds_in_move_step": round(total["move_seconds"], 3),
            "contender_score": {"wins": total["wins"], "draws": total["draws"], "losses": total["losses"]},
            "workload": "arena between two RISEv2-13 80-channel nets (native loop), 3check then king-of-the-hill, 128 concurrent games in colour-"
                        "swapped pairs from the variants' opening positions, both players searching at the same time, batch 1024 shared by the "
                        "running trees, 400 simulations per move, ply cap 80"}
        for v in res_.values():
            v["precision"] = prec
        return res_

    out = legs(args.precision)
    other = getattr(args, "search_precision_other", None) if other_mode else None
    if other and other != args.precision:                                # the same games with nets of the other mode, beside the line's
        for k, v in legs(other).items():
            out[k][f"games_per_min_{other}"] = v["games_per_min"]
            out[k][f"mcts_nodes_per_sec_{other}"] = v["mcts_nodes_per_sec"]
    return out


LINE_LIMIT = 6144      # bytes of the ONE stdout line: the driver's record parser lost round 4's 21.7 KB line


def compact_record(full, detail_path):
    """The stdout line from the whole result: the contract's keys, `roofline` (scalars + `pmc` + `per_op_ms`), `cpu_baseline` (scalars)
    and a flat `summary` of the companion rates; everything else -- per-mode blocks, search / game / drop-in legs, sweeps -- stays in
    the detail file whose path the line carries.  Pure (no GPU): tests/test_bench_record.py feeds it a canned result."""
    line = {k: full[k] for k in ("metric", "value", "value_precision", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data", "config") if k in full}
    rf = full["roofline"]
    keep = ("bound", "kernel", "launches_per_step", "avg_launch_ms", "achieved", "peak", "unit", "frac", "frac_of_dense_f16_peak", "peak_definition", "traffic",
            "traffic_unit", "traffic_source", "pmc", "per_op_ms")
    line["roofline"] = {k: rf[k] for k in keep if k in rf}
    if "whole_forward" in rf:
        line["roofline"]["whole_forward_ms"] = rf["whole_forward"].get("ms_per_step", rf["whole_forward"].get("event_ms_per_step"))
        line["roofline"]["whole_forward_frac"] = rf["whole_forward"]["frac"]
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample", "value_q1", "value_q3", "iqr_over_median",
                                                   "n_samples", "cpu_model", "mcts_nodes_per_sec") if k in cb}
        ref1 = cb.get("config1_reference_search", {})
        if "mcts_nodes_per_sec" in ref1:
            line["cpu_baseline"]["config1_reference_search_nodes_per_sec"] = ref1["mcts_nodes_per_sec"]
    tr = full.get("timed_region")
    if tr:
        line["timed_region"] = {k: tr[k] for k in ("repeats", "ms_per_step_min", "ms_per_step_max") if k in tr}
    summary = {"nn_evals_per_sec": full["value"], "precision": full.get("value_precision")}
    if "frac" in rf:                                                     # (the dominant kernel's roofline: --full only)
        summary["roofline_frac"] = rf["frac"]
    for m_, r_ in full.get("modes", {}).items():
        if "evals_per_sec" in r_:                                        # (a leg that recorded a skip or an error has no rate)
            summary[f"nn_evals_per_sec_{m_}"] = r_["evals_per_sec"]
            summary[f"frac_of_peak_{m_}"] = r_.get("frac")
    pcie = full.get("pcie_inclusive")
    if pcie:
        # SURVEY 8(d) Metric 1 as the reference's `inference` command computes it (crazyara.cpp:156-181: the host copies included), at the top
        # level beside `value` (which the bench contract defines as device-resident: inputs in HBM when the timed region starts)
        line["value_device_resident"] = full["value"]
        line["value_pcie_inclusive_one_user"] = pcie["one_net_evals_per_sec"]
        line["value_pcie_inclusive_two_users"] = pcie["two_nets_in_flight_evals_per_sec"]
        summary["pcie_inclusive_one_user"] = pcie["one_net_evals_per_sec"]
        summary["pcie_inclusive_two_users"] = pcie["two_nets_in_flight_evals_per_sec"]
        for k_ in ("copy_path_one_net_evals_per_sec", "copy_path_two_nets_evals_per_sec", "zero_copy_forced_two_nets_evals_per_sec"):
            if k_ in pcie:
                summary[k_.replace("_evals_per_sec", "").replace("_net", "_user")] = pcie[k_]
    for k_, r_ in (full.get("nn_by_batch") or {}).items():
        summary[f"nn_evals_per_sec_{k_}"] = r_["evals_per_sec"]
    mcts = full.get("mcts")
    if mcts:
        summary[f"config2_mcts_nodes_per_sec_{mcts['precision']}"] = mcts["mcts_nodes_per_sec"]
        summary["config2_batch_fill"] = mcts.get("avg_batch_fill")
        summary["config2_host_throttled_ms"] = mcts.get("host_cgroup_throttled_ms_during_search")
        for th_, v_ in mcts.get("nodes_per_sec_by_host_threads", {}).items():
            summary[f"config2_nodes_per_sec_{th_}_host_threads"] = v_
        if "predicted_8_gpus" in mcts:
            summary["predicted_8_gpus_nodes_per_sec"] = mcts["predicted_8_gpus"]["mcts_nodes_per_sec"]
        if "per_rank_nodes_per_sec" in mcts:
            summary["per_rank_nodes_per_sec"] = mcts["per_rank_nodes_per_sec"]
    other = full.get("mcts_other_mode")
    if other:
        summary[f"config2_mcts_nodes_per_sec_{other['precision']}"] = other["mcts_nodes_per_sec"]
    for k_, r_ in (full.get("mcts_configs") or {}).items():
        if "mcts_nodes_per_sec" not in r_:
            continue
        summary[f"{k_}_nodes_per_sec"] = r_["mcts_nodes_per_sec"]
        if k_.startswith("config2_one_tree") and "avg_batch_fill" in r_:
            summary[f"{k_}_fill"] = r_["avg_batch_fill"]
        for kk_, v_ in r_.items():                                   # the same leg with nets of the other mode
            if kk_.startswith("mcts_nodes_per_sec_"):
                summary[f"{k_}_nodes_per_sec_{kk_[len('mcts_nodes_per_sec_'):]}"] = v_
    for k_, r_ in (full.get("game_configs") or {}).items():
        if "games_per_min" not in r_:
            continue
        summary[f"{k_}_nodes_per_sec"] = r_.get("mcts_nodes_per_sec")
        summary[f"{k_}_games_per_min"] = r_["games_per_min"]
        for kk_, v_ in r_.items():
            if kk_.startswith("games_per_min_"):
                summary[f"{k_}_{kk_}"] = v_
        if "per_rank_games_per_min" in r_:
            summary[f"{k_}_per_rank_games_per_min"] = r_["per_rank_games_per_min"]
    dropin = full.get("dropin_reference_search")
    if dropin and "skipped" not in dropin:
        for k_, r_ in dropin.items():
            if isinstance(r_, dict) and "config2_mcts_nodes_per_sec" in r_:
                summary[f"dropin_config2_nodes_per_sec_{k_}"] = r_["config2_mcts_nodes_per_sec"]
    if cb:
        summary["cpu_evals_per_sec"] = cb["value"]
        summary["cpu_cores"] = cb["cores"]
    summary["bench_seconds"] = full.get("bench_seconds")
    line["detail"] = detail_path
    line["summary"] = summary
    # the line must stay under the limit whatever legs ran: drop the least important summary keys first, then long strings
    def size():
        return len(json.dumps(line))
    for victim in ("dropin_", "frac_of_peak_", "config1_", "config2_one_tree", "benchmark_positions", "config2_nodes_per_sec_", "copy_path_"):
        if size() < LINE_LIMIT:
            break
        for k_ in [k_ for k_ in summary if k_.startswith(victim)]:
            del summary[k_]
    if size() >= LINE_LIMIT:
        line["roofline"].pop("per_op_ms", None)
        line.get("cpu_baseline", {}).pop("sample", None)
    if size() >= LINE_LIMIT:
        line["roofline"].pop("pmc", None)
        line["roofline"].pop("peak_definition", None)
    # last resort: the summary's remaining companion keys go, least important (longest-named) first; the contract's keys, roofline and
    # cpu_baseline scalars stay -- the limit holds whatever legs ran
    for k_ in sorted([k_ for k_ in summary if k_ not in ("nn_evals_per_sec", "precision", "roofline_frac")], key=len, reverse=True):
        if size() < LINE_LIMIT:
            break
        del summary[k_]
    return line


def respawn_one_rank_per_gpu(n):
    """`python bench.py --gpus N` started plainly (no WORLD_SIZE in the environment): become N ranks, one per GPU, by re-executing this
    command under torch.distributed.run -- the same launch line the contract names (rl_loop.py:60: one process per GPU)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execv(sys.executable, cmd)


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 20240


def device_outputs(net):
    """What a forward leaves for its caller in the net's device buffers (value, policy probabilities, auxiliary outputs), on the host."""
    torch.cuda.synchronize()
    return {name: torch.as_tensor(view, device="cuda").cpu().numpy()
            for name, view in net.device_buffers().items() if name in ("value", "probs", "aux")}


def write_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """arrays (name -> [batch, ...]) as <out_dir>/<name>.npy in float32.  Above `limit` bytes in all, every array keeps the same seeded
    sample of boards, whose indices go to boards.npy (float64), so that two runs with the same arguments write the same boards."""
    arrays = {name: np.ascontiguousarray(a, dtype=np.float32) for name, a in arrays.items()}
    batch = next(iter(arrays.values())).shape[0]
    per_board = sum(a.nbytes for a in arrays.values()) // batch
    if per_board * batch > limit:
        keep = limit // (per_board + 8)
        boards = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(batch, size=keep, replace=False))
        arrays = {name: a[boards] for name, a in arrays.items()}
        arrays["boards"] = boards.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return arrays


def timed_mode_leg(local_rank, batch, model_dir, precision, x, steps, flops_peak):
    """One more precision mode on the same workload (N = 1 information, never `value`): evals/s, ms per step, achieved TFLOP/s."""
    from crazyara_amd.neuralnetapi import HipAPI
    net = HipAPI(local_rank, batch, model_dir, precision)
    torch.as_tensor(net.device_buffers()["planes"], device="cuda").copy_(x.cuda())
    torch.cuda.synchronize()
    for _ in range(5):
        net.forward_device()
    net.sync()
    t = time.perf_counter()
    for _ in range(steps):
        net.forward_device()
    net.sync()
    el = time.perf_counter() - t
    agg = {}
    for name, ms in net.time_ops(3):
        agg[name] = agg.get(name, 0.0) + ms
    tf = net.flops_per_position() * batch * steps / el / 1e12
    out = {"evals_per_sec": round(steps * batch / el, 1), "ms_per_step": round(el / steps * 1e3, 4), "steps": steps,
           "achieved": round(tf, 2), "peak": flops_peak, "unit": "TFLOP/s", "frac": round(tf / flops_peak, 4),
           "per_op_ms": {k: round(v, 4) for k, v in agg.items()}}
    return net, out


def main():
    t_bench_start = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--precision", default="float16x3", choices=["float16x3", "float16p8", "float16", "float32"],
                    help="the headline mode.  float16x3 (default since round 6): split-operand f16 MFMAs, f32-grade products -- logits within 1e-3 of "
                         "fp32 up to logits of +-25 (7e-6 on the seeded nets, 1.3e-4 at +-10, 5e-4 at +-25: profiles/r06/h_*).  float16p8: float16x3 whose tower takes the cross "
                         "terms of its two 1x1 GEMMs through e5m2 MFMAs: 20 %% faster, but its error is relative to the activations -- "
                         "<= 2.5e-4 x max|logit|, i.e. inside 1e-3 on the seeded nets (max|logit| ~ 2: round 5's headline) and OUTSIDE it on nets with "
                         "trained-size logits (tests/test_nn_parity_gpu.py::test_float16p8_error_grows_with_the_logit_scale_float16x3_holds); float16: the "
                         "reference's TensorRT default (its logits miss 1e-3 by 2-3x); float32: exact-f32 MFMA")
    ap.add_argument("--blocks", type=int, default=N_BLOCKS)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed region, write what its last step computed (value, policy probabilities, auxiliary outputs: what "
                         "a caller of the path receives) as DIR/<name>.npy in float32, at most 64 MB in all; with the same arguments the "
                         "inputs are the same from run to run, so that two builds can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run everything else the benchmark measures: the other precision modes and batch "
                         "sizes, the PCIe-inclusive rates, the per-kernel roofline with its live PMC passes, the search / game / drop-in "
                         "legs and the CPU baseline (the --no-* options and --timed-only leave some of them out).  Without it the line "
                         "carries the headline and the whole forward's roofline on the timed region's clock")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--simulations", type=int, default=1600)
    ap.add_argument("--search-quota", type=int, default=16, help="leaves per tree per batch (reference Batch_Size default 16)")
    ap.add_argument("--search-threads", type=int, default=16)
    ap.add_argument("--search-lanes", type=int, default=2, help="batches in flight (the reference: one per SearchThread, Threads default 2)")
    ap.add_argument("--search-precision", default="headline",
                    help="precision of the nets behind the search legs; `headline` (default) = the mode of --precision, so that the nodes/sec "
                         "of the line are those of the conformant mode; the config-2 leg also runs once with --search-precision-other")
    ap.add_argument("--search-precision-other", default="float16",
                    help="second precision of the config-2 search leg (the reference's TensorRT default: value / priors within 1e-3 / 1e-5 of "
                         "fp32, logits non-conformant), reported as config2_mcts_nodes_per_sec_<mode>")
    ap.add_argument("--no-dropin-leg", action="store_true", help="skip the reference-MCTSAgent-on-HipAPI throughput leg")
    ap.add_argument("--dry-ranks", action="store_true",
                    help="rehearsal of the N-rank launch on a box with ONE GPU: every rank binds to device 0, rank 0 runs its legs, ranks "
                         "1..N-1 skip the compute and take part in every rendezvous, barrier, reduce and gather.  RCCL is tried with the "
                         "shared device; when it refuses (duplicate GPU) the collectives run over gloo and the line says so.  The numbers "
                         "of such a run are those of N = 1; it exists so that the multi-rank path has run on hardware before a node does")
    ap.add_argument("--search-seconds", type=float, default=1.0, help="minimum timed region of one repeat of a search leg")
    ap.add_argument("--search-repeats", type=int, default=3)
    ap.add_argument("--no-config-legs", action="store_true", help="skip the search legs of BASELINE configs 1, 3, 4, 5")
    ap.add_argument("--no-live-pmc", action="store_true", help="roofline.traffic from the newest committed PMC pass instead of live passes")
    ap.add_argument("--detail-out", default="bench_detail.json",
                    help="file that receives the WHOLE result (per-mode blocks, search / game / drop-in legs, sweeps); the stdout line keeps the "
                         "contract's keys + roofline + cpu_baseline + a flat summary and stays under 6 KB")
    ap.add_argument("--timed-only", action="store_true",
                    help="with --full: only the headline's timed region and its per-kernel events: no other modes / PCIe / search / CPU legs, "
                         "no PMC child passes (the command scripts/gpu_round.sh runs under rocprofv3 --kernel-trace --stats, so that the "
                         "trace holds nothing but the launches the roofline is quoted on)")
    args = ap.parse_args()
    if args.timed_only:
        args.no_search = args.no_cpu_baseline = args.no_live_pmc = True
    if args.search_precision == "headline":
        args.search_precision = args.precision

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_one_rank_per_gpu(args.gpus)          # does not return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path is the HIP library, there is no CPU fallback")
    # stdout carries ONE line, the JSON record: whatever the libraries of this process print on file descriptor 1 on the way (gloo's
    # "[Gloo] Rank ... is connected", RCCL's version banner) goes to stderr instead
    sys.stdout.flush()
    record_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    if args.gpus != world:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: the launcher's rank count and --gpus must agree")
    dry = bool(args.dry_ranks) and rank > 0                 # a rehearsal rank: every collective, no compute
    if args.dry_ranks:
        local_rank = 0                                      # every rank on the one GPU
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} GPU(s) visible -- refusing to "
                         f"share a GPU between replicas (the numbers would mean nothing; --dry-ranks rehearses the launch on one GPU)")
    torch.cuda.set_device(local_rank)
    dist = None
    collective_backend = None
    if world > 1:
        import torch.distributed as dist
        if not args.dry_ranks:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            collective_backend = "nccl"
        else:
            # gloo carries the rehearsal whatever happens; RCCL is tried on a second group over the shared device and its verdict
            # (agreed over gloo, so that every rank takes the same branch) decides which group the collectives below use
            dist.init_process_group("gloo", rank=rank, world_size=world)
            ok, why = 1, ""
            try:
                g = dist.new_group(backend="nccl")
                t = torch.ones(1, device="cuda")
                dist.all_reduce(t, group=g)
                torch.cuda.synchronize()
                ok = int(float(t.item()) == float(world))
            except Exception as e:  # noqa: BLE001 -- RCCL refuses ranks that share a device
                ok, why = 0, repr(e)[:300]
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            collective_backend = "nccl (shared device)" if int(flag.item()) == 1 else "gloo (RCCL refused the shared device: " + (why or "on another rank") + ")"
            if int(flag.item()) == 1:
                nccl_group = g
                _all_reduce, _all_gather, _barrier = dist.all_reduce, dist.all_gather, dist.barrier

                class _OnNccl:                               # the same three calls, on the nccl group
                    ReduceOp = dist.ReduceOp
                    is_initialized = staticmethod(dist.is_initialized)
                    get_world_size = staticmethod(dist.get_world_size)
                    destroy_process_group = staticmethod(dist.destroy_process_group)

                    @staticmethod
                    def all_reduce(t_, op=dist.ReduceOp.SUM):
                        return _all_reduce(t_, op=op, group=nccl_group)

                    @staticmethod
                    def all_gather(l_, t_):
                        return _all_gather(l_, t_, group=nccl_group)

                    @staticmethod
                    def barrier():
                        return _barrier(group=nccl_group)
                dist = _OnNccl

    from crazyara_amd import build, netfile, replicas, rise_config
    from crazyara_amd.neuralnetapi import HipAPI
    if local_rank == 0:
        build.build()
    if dist is not None:
        dist.barrier()

    cfg = rise_config.rise_v2_config(args.blocks, 34, 81)
    sd = rise_config.make_state_dict(cfg, seed=2024, stress=True)
    tmp = tempfile.mkdtemp(prefix=f"cra_bench_{rank}_")
    netfile.export_rise(os.path.join(tmp, f"{cfg.name}-v1.0.cranet"), cfg, sd, input_version="1.0")
    net = HipAPI(local_rank, args.batch, tmp, args.precision)
    x = synthetic_planes(args.batch, cfg.nb_input_channels, seed=7 + rank)
    bufs = net.device_buffers()
    torch.as_tensor(bufs["planes"], device="cuda").copy_(x.cuda())
    torch.cuda.synchronize()
    dev = torch.device("cuda", local_rank)
    if collective_backend is not None and collective_backend.startswith("gloo"):
        dev = torch.device("cpu")                           # gloo reduces host tensors

    def sync_all():
        net.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def timed_region():
        """EXACTLY --steps steps between barrier + synchronize on both sides; seconds = MAX over the ranks (the only collective of the
        NN leg besides the SUM of evaluations)."""
        sync_all()
        t0 = time.perf_counter()
        if not dry:
            for _ in range(args.steps):
                net.forward_device()
        net.sync()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        ev, el, _ = replicas.reduce_stats(replicas.ReplicaStats(units=0.0 if dry else float(args.steps * args.batch), seconds=el), dist, dev)
        return ev, el

    for _ in range(0 if dry else args.warmup):
        net.forward_device()
    # one region of exactly --steps steps: a short request is a noisy one, and the caller chooses its length
    evals, elapsed = timed_region()
    regions = [elapsed]
    if dist is not None:
        dist.barrier()
    value = evals / elapsed
    if args.dump_outputs and rank == 0:
        written = write_outputs(args.dump_outputs, device_outputs(net))
        print(f"bench: the last timed step's outputs written to {args.dump_outputs}: "
              + ", ".join(f"{k} {list(a.shape)}" for k, a in written.items()), file=sys.stderr)

    # ---- MCTS leg (BASELINE config 2: batch 256, 1600 simulations per search, fixed opening set) ----
    # Timed region >= 1 s: rounds of "every tree restarts from its next opening position and is searched to 1600 simulations" until
    # the pool's own run times add up to a second; median / min / max over three such repeats (crazyara_amd/searchbench.py).
    mcts = None
    mcts_headline_mode = None
    mcts_configs = None
    game_configs = None
    dropin = None
    if args.full and not args.no_search:
        from crazyara_amd import openings, search, searchbench
        lanes = max(1, args.search_lanes)
        st = search.default_settings(mode=0, version_major=1, batch_size=args.search_quota)
        n_trees = lanes * max(1, args.batch // args.search_quota)
        # the fixed crazyhouse opening set: the 50 openings of zh-50_startpos.pgn + every position of the two calibration games
        positions = [(f, False, "crazyhouse") for f in openings.crazyhouse_opening_set()]
        # host budget of this rank: its slice of the node's CPUs (near its GPU when the topology is known), threads <= that slice.
        # `threads` counts the driving thread; one tree of a lane per thread is the fastest split, so with 16 trees per lane anything
        # below 16 makes one thread do two trees per batch
        cpus_avail = replicas.available_cpus()
        _, budget_threads = replicas.pin_rank_to_cpus(world, int(os.environ.get("LOCAL_RANK", "0")), use_gpu_topology=not args.dry_ranks)
        threads = max(1, min(args.search_threads, budget_threads))

        def config2_leg(precision, repeats, leg_threads=None):
            if dry:                                         # rehearsal rank: no search, every collective
                nets, leg = [], {"_median_totals": (0, 0, 0, 1e-9), "_spread": None}
            else:
                nets = [HipAPI(local_rank, args.batch, tmp, precision) for _ in range(lanes)]
                leg = searchbench.timed_search_leg(st, nets, positions, n_trees, args.simulations, leg_threads or threads,
                                                   min_seconds=args.search_seconds, repeats=repeats, offset=rank * 37)
            nodes_m, evals_m, sims_m, sec_m = leg.pop("_median_totals")
            leg.pop("_spread")
            # RCCL sum of {nodes, evals, simulations}, max of seconds over the ranks' median repeats
            nodes_t, sec_t, ex = replicas.reduce_stats(replicas.ReplicaStats(units=float(nodes_m), seconds=sec_m,
                                                                               extra=(float(evals_m), float(sims_m))), dist, dev)
            r = dict(leg)
            r.update({"mcts_nodes_per_sec": round(nodes_t / sec_t, 1), "mcts_nn_evals_per_sec": round(ex[0] / sec_t, 1),
                      "simulations_per_sec": round(ex[1] / sec_t, 1), "seconds": round(sec_t, 3), "per_tree_quota": args.search_quota,
                      "host_cpus_available": cpus_avail, "precision": precision,
                      "workload": "BASELINE config 2: crazyhouse opening set, RISEv2-19, batch 256, 1600 simulations per tree"})
            if world > 1:
                # every rank's own rate next to the aggregate: a host-starved rank is visible (one more all_gather of a scalar)
                mine = torch.tensor([nodes_m / sec_m, float(threads)], dtype=torch.float64, device=dev)
                allr = [torch.zeros_like(mine) for _ in range(world)]
                dist.all_gather(allr, mine)
                r["per_rank_nodes_per_sec"] = [round(float(v[0]), 1) for v in allr]
                r["per_rank_host_threads"] = [int(v[1]) for v in allr]
            return nets, r

        nets, mcts = config2_leg(args.search_precision, args.search_repeats)
        if len(nets) > 1 and world == 1:
            # informational: two batches of 256 in flight, as two SearchThreads of the reference keep them (own weights, own stream
            # each).  Never `value`.
            import threading
            half = max(1, args.steps // 2)
            for n2 in nets[:2]:
                torch.as_tensor(n2.device_buffers()["planes"], device="cuda").copy_(x.cuda())
                n2.forward_device()
                n2.sync()

            def replay(n2):
                for _ in range(half):
                    n2.forward_device()
                n2.sync()
            ths = [threading.Thread(target=replay, args=(n2,)) for n2 in nets[:2]]
            t2 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            mcts["nn_two_batches_in_flight_evals_per_sec"] = round(2 * half * args.batch / (time.perf_counter() - t2), 1)
        for n_ in nets:
            n_.close()
        if args.search_precision_other and args.search_precision_other != args.search_precision:
            nets, mcts_headline_mode = config2_leg(args.search_precision_other, 1)       # the same leg in the other mode (one repeat)
            for n_ in nets:
                n_.close()
        if world == 1 and not args.no_config_legs:
            # how many host threads a GPU needs (searchthread.cpp runs `Threads` of them per GPU): the same leg with fewer
            sweep = {}
            for th in (1, 2, 4, 8):
                if th < threads:
                    nets, r_ = config2_leg(args.search_precision, 1, leg_threads=th)
                    sweep[str(th)] = r_["mcts_nodes_per_sec"]
                    for n_ in nets:
                        n_.close()
            sweep[str(threads)] = mcts["mcts_nodes_per_sec"]
            mcts["nodes_per_sec_by_host_threads"] = sweep
            # what 8 ranks on this host would get: each rank its eighth of the CPUs this process may use (replicas.pin_rank_to_cpus)
            per_rank = max(1, cpus_avail // 8)
            usable = max((int(k) for k in sweep if int(k) <= per_rank), default=min(int(k) for k in sweep))
            mcts["predicted_8_gpus"] = {"host_cpus": cpus_avail, "host_threads_per_rank": per_rank, "sweep_point_used": usable,
                                        "mcts_nodes_per_sec": round(8 * sweep[str(usable)], 1),
                                        "note": "8 x the one-GPU rate at the host-thread count an eighth of this host's CPUs gives a rank; "
                                                "the GPUs do not interact (replicas), the host is the shared resource"}
        # ---- the other BASELINE configurations, searched (single GPU; extra keys, never `value`) ----
        if world == 1 and not args.no_config_legs:
            cargs = argparse.Namespace(**vars(args))
            cargs.precision = args.search_precision
            mcts_configs = config_search_legs(cargs, local_rank, threads)
            game_configs = config_game_legs(cargs, local_rank, threads)
        if world == 1 and not args.no_dropin_leg:
            dropin = dropin_reference_search(tmp, local_rank, args.batch, precisions=(args.search_precision, "float16") if args.search_precision != "float16" else ("float16",))
        if world > 1 and not args.no_config_legs:
            # BASELINE configs 4 and 5 are DEFINED on several GPUs (chess960 self-play games and the 3check / KOTH arena sharded over the
            # node): every rank plays its share of the games, one all_reduce of {games, moves, nodes} (SUM) and seconds (MAX) per leg --
            # the reduction rl_loop.py's driver does over its per-device files (rl/rl_loop.py:60, selfplay.cpp:339-351).  Fewer games per
            # rank than the N = 1 legs so that the whole run stays inside minutes on a host that 8 ranks share.
            cargs = argparse.Namespace(**vars(args))
            cargs.precision = args.search_precision
            if dry:
                mine = {}
            else:
                mine = config_game_legs(cargs, local_rank, threads, rank=rank, world=world, selfplay_games=8, arena_games=32, other_mode=False)
            game_configs = {}
            for key in ("config4_selfplay_one_gpu", "config5_arena_one_gpu"):
                r_ = replicas.reduce_game_leg(mine.get(key), dist, dev, world)
                r_["precision"] = args.search_precision
                r_["workload"] = (mine.get(key, {}).get("workload") or "") + f" -- sharded over {world} ranks, game g -> rank g % {world}"
                game_configs[key.replace("_one_gpu", "")] = r_

    out = None
    if rank == 0:
        flops_total = net.flops_per_position() * args.batch
        # float16x3: a product costs three f16 MFMAs, so the ceiling of ALGORITHMIC FLOP/s is a third of the dense f16 peak
        # float16p8: both GEMMs of the tower cost one f16 MFMA + two e5m2 products at twice the f16 rate per product = two f16 equivalents
        peak = {"float16": PEAK_F16_TFLOPS, "float16x3": PEAK_F16_TFLOPS / 3.0, "float16p8": PEAK_F16_TFLOPS / 2.0,
                "float32": PEAK_F32_TFLOPS}[args.precision]
        peak_definition = {"float16": "dense f16 MFMA peak", "float32": "exact-f32 MFMA peak",
                           "float16x3": "dense f16 peak / 3 (three f16 MFMAs per product)",
                           "float16p8": "dense f16 peak / 2 (one f16 MFMA + two e5m2 products at the 5 PFLOP/s 8-bit peak per product)"}[args.precision]
        # the whole forward on the SAME clock as ms_per_step (the timed region); --full adds the event-timed replay beside it
        whole_forward = {"ms_per_step": round(elapsed / args.steps * 1e3, 4),
                         "achieved": round(flops_total / (elapsed / args.steps) / 1e12, 2),
                         "frac": round(flops_total / (elapsed / args.steps) / 1e12 / peak, 4)}
        roofline = {"peak": round(peak, 1), "unit": "TFLOP/s", "peak_definition": peak_definition, "whole_forward": whole_forward}
        if args.full:
            # ---- roofline of the dominant kernel, timed live with hipEvents on the net's own stream ----
            # (at least 200 replays in front of the per-launch timing, whatever --steps says: the rank has just spent tens of seconds in host-side
            # legs, and five launches on a chip that has clocked down read 5 % long -- 0.615 ms against 0.583 for the tower with --steps 20,
            # profiles/r06/I_bench_steps20.json; the timed region above is not touched by this)
            settle = max(args.steps, 200)
            ev_ms = net.time_forward(settle) / settle
            ops = net.time_ops(10)
            agg, cnt = {}, {}
            for name, ms in ops:
                agg[name] = agg.get(name, 0.0) + ms
                cnt[name] = cnt.get(name, 0) + 1
            dom = max(agg, key=agg.get)
            # algorithmic FLOPs of the dominant kernel's launches (1x1 expand/project GEMMs + depthwise of all blocks)
            cops = cfg.channels_operating()
            if dom in ("fused_block", "tower", "block_x3", "tower_x3", "tower_p8"):
                dom_flops = sum(2.0 * 64 * c * (2 * cfg.channels + 9) for c in cops) * args.batch
            elif dom == "conv_gemm_1x1":
                dom_flops = sum(2.0 * 64 * cfg.channels * c * 2 for c in cops) * args.batch
            elif dom == "conv_gemm_3x3":
                dom_flops = 2.0 * 64 * 9 * (cfg.nb_input_channels * 256 + 256 * 256 + 256 * cfg.channels_policy_head) * args.batch
            else:
                dom_flops = flops_total
            per_op_three = None
            if dom == "forward":
                # the whole forward is one launch (forward.hip); the same net as three launches gives the split per stage (informational)
                net3 = HipAPI(local_rank, args.batch, tmp, args.precision + "-3k")
                torch.as_tensor(net3.device_buffers()["planes"], device="cuda").copy_(x.cuda())
                net3.time_ops(2)
                a3 = {}
                for name, ms in net3.time_ops(5):
                    a3[name] = a3.get(name, 0.0) + ms
                per_op_three = {k: round(v, 4) for k, v in a3.items()}
                net3.close()
            dom_ms = agg[dom]                                              # all launches of the dominant kernel in ONE step (time_ops: per-launch averages)
            achieved = dom_flops / (dom_ms * 1e-3) / 1e12
            traffic = None if (args.no_live_pmc or world > 1) else live_pmc_traffic(dom, args.blocks, args.batch, args.precision)
            if traffic is None:
                traffic = committed_pmc_traffic(dom)
            whole_forward["event_ms_per_step"] = round(ev_ms, 4)
            roofline = {"bound": "mfma", "kernel": dom, "launches_per_step": cnt[dom],
                        "avg_launch_ms": round(dom_ms / cnt[dom], 5), "achieved": round(achieved, 2), "peak": round(peak, 1),
                        "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                        "frac_of_dense_f16_peak": round(achieved / PEAK_F16_TFLOPS, 4),
                        "peak_definition": peak_definition,
                        **traffic,
                        "whole_forward": whole_forward,
                        "per_op_ms": {k: round(v, 4) for k, v in agg.items()}}
            if per_op_three:
                roofline["per_op_ms_as_three_launches"] = per_op_three
        # ---- the same workload in the other precision modes (N = 1 information, never `value`) ----
        #   float16   : the reference's TensorRT default (optionsuci.cpp:143-147); predict()'s outputs meet 1e-3, its logits do not
        #   float32   : exact-f32 MFMA (v_mfma_f32_16x16x4_f32), the slow mode that meets 1e-3 on the logits
        #   fp8       : e4m3 operands in the tower's GEMMs, the counterpart of the reference's INT8 mode
        single = args.full and world == 1 and not args.timed_only
        modes = {}
        if single:
            for mode, mpeak, msteps in (("float16", PEAK_F16_TFLOPS, max(30, args.steps)), ("float16x3", PEAK_F16_TFLOPS / 3.0, max(20, args.steps // 2)),
                                        ("float16p8", PEAK_F16_TFLOPS / 2.0, max(20, args.steps // 2)),
                                        ("float32", PEAK_F32_TFLOPS, max(10, args.steps // 6)), ("fp8", PEAK_FP8_TFLOPS, max(30, args.steps // 2)),
                                        ("int8", PEAK_FP8_TFLOPS, max(30, args.steps // 2))):       # (i8 MFMAs run at the 8-bit rate: 2 x K of f16)
                if mode == args.precision:
                    continue
                mnet, modes[mode] = timed_mode_leg(local_rank, args.batch, tmp, mode, x, msteps, round(mpeak, 1))
                if mode in ("fp8", "int8"):
                    xin = np.ascontiguousarray(x.numpy()).reshape(-1)
                    v8 = np.zeros(args.batch, np.float32); p8 = np.zeros(args.batch * cfg.nb_policy, np.float32)
                    vh = np.zeros(args.batch, np.float32); ph = np.zeros(args.batch * cfg.nb_policy, np.float32)
                    mnet.predict(xin, v8, p8)
                    net.predict(xin, vh, ph)
                    modes[mode].update({"share_of_flops_in_8bit": round(876.6 / 1002.6, 3) if args.blocks == N_BLOCKS else None,
                                        "operands": ("e4m3 in the expand / project GEMMs of the residual tower (v_mfma_f32_32x32x64_f8f6f4), f16 elsewhere" if mode == "fp8" else
                                                     "calibrated int8 in the expand / project GEMMs of the residual tower (v_mfma_i32_32x32x32_i8; one step per "
                                                     "activation tensor and block from the reference's calibration games, one per weight row), f16 elsewhere"),
                                        "max_abs_diff_vs_headline_mode": {"value": round(float(np.abs(v8 - vh).max()), 5),
                                                                          "prob": round(float(np.abs(p8 - ph).max()), 7)}})
                mnet.close()
            notes = {"float16": "the reference's TensorRT default; value / probabilities within 1e-3 / 1e-5 of fp32, logits 1e-3 ... 3.3e-3 (non-conformant)",
                     "float16x3": "logits within 1e-4 of fp32 on the seeded nets (measured 7e-6), 1.3e-4 at logits of +-10, inside 1e-3 up to +-25: conformant",
                     "float16p8": "logit error <= 2.5e-4 x max|logit|: within 1e-3 on the seeded nets (max|logit| ~ 2; 7e-4 over 5.5 million logits), outside it at trained-net logit scales",
                     "float32": "logits within 1e-4 of fp32 (measured 5e-6): conformant",
                     "fp8": "reduced precision, e4m3 operands: value 1 - 3e-2 from fp32, not conformant",
                     "int8": "the reference's Precision int8 (calibrated INT8): value 6 - 8e-3 from fp32 (tests/test_int8.py), not conformant"}
            for m_ in modes:
                modes[m_]["logit_tolerance"] = notes[m_]
        # ---- SURVEY 8(d) Metric 1's other batch sizes (8 / 512 / 1024, device-resident, headline mode) and config 3's net with both value
        # heads (tanh and WDLP: the released ClassicAra net is the WDLP variant) at its batch of 512 ----
        nn_by_batch = {}
        if single:
            for bsz in (8, 512, 1024):
                xb_ = synthetic_planes(bsz, cfg.nb_input_channels, seed=11)
                n_, r_ = timed_mode_leg(local_rank, bsz, tmp, args.precision, xb_, max(20, args.steps // (1 if bsz == 8 else 4)), round(peak, 1))
                n_.close()
                nn_by_batch[f"batch{bsz}"] = {k: r_[k] for k in ("evals_per_sec", "ms_per_step", "frac")}
            for tag, wdl in (("config3_tanh", False), ("config3_wdlp", True)):
                cfg3 = rise_config.rise_v33_config(52, 76, wdl)
                sd3 = rise_config.make_state_dict(cfg3, seed=31, stress=True)
                d3 = tempfile.mkdtemp(prefix="cra_bench_c3_")
                netfile.export_rise(os.path.join(d3, f"{cfg3.name}-v3.0.cranet"), cfg3, sd3, input_version="3.0")
                n_, r_ = timed_mode_leg(local_rank, 512, d3, args.precision, synthetic_planes(512, 52, seed=12), max(20, args.steps // 4), round(peak, 1))
                n_.close()
                nn_by_batch[tag] = {k: r_[k] for k in ("evals_per_sec", "ms_per_step", "frac")}
                nn_by_batch[tag]["workload"] = f"chess RISEv3.3 (52x8x8 -> 4864 + value{' WDLP + 4 aux' if wdl else ' tanh'}), batch 512"
        # ---- PCIe-inclusive rate: the reference's `inference` command (crazyara.cpp:156-181) = back-to-back blocking predict() on the
        # NeuralNetAPIUser's pinned buffers, planes in and value / probabilities out through PCIe on every call.  With pinned buffers
        # predict issues no copy commands (kernels read / write the host buffers in place); the copy path is timed beside it, and two
        # users on two nets (two SearchThreads, crazyara.cpp:548-563) show what the engine gets with its default Threads = 2. ----
        import threading
        from crazyara_amd.neuralnetapi import NeuralNetAPIUser
        it = max(400, args.steps)          # >= 0.25 s per leg: 150 iterations (0.1 s) made the legs swing by 10 % between runs (round 6)

        def pcie_rate(nets_):
            users = [NeuralNetAPIUser([n_]) for n_ in nets_]
            for u in users:
                u.input_planes[:] = x.numpy().reshape(-1)
                u.run_inference(5)
            ths = [threading.Thread(target=u.run_inference, args=(it,)) for u in users]
            t1 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            el = time.perf_counter() - t1
            zc = all(n_.last_submit_zero_copy() for n_ in nets_)
            for u in users:
                u.close()
            return len(users) * it * args.batch / el, zc
        pcie, pcie_rate_1 = None, None
        if single:
            net_b = HipAPI(local_rank, args.batch, tmp, args.precision)
            pcie_rate_1, zc1 = pcie_rate([net])
            pcie_rate_2, zc2 = pcie_rate([net, net_b])
            os.environ["CRA_PREDICT_COPY"] = "1"                 # read when a net is made: the copy path runs on nets of its own
            net_c, net_d = HipAPI(local_rank, args.batch, tmp, args.precision), HipAPI(local_rank, args.batch, tmp, args.precision)
            del os.environ["CRA_PREDICT_COPY"]
            pcie_copy_1, _ = pcie_rate([net_c])
            pcie_copy_2, _ = pcie_rate([net_c, net_d])
            net_c.close()
            net_d.close()
            os.environ["CRA_PREDICT_ZERO_COPY"] = "1"            # round 5's default for two users, for the A/B beside the new one
            net_e, net_f = HipAPI(local_rank, args.batch, tmp, args.precision), HipAPI(local_rank, args.batch, tmp, args.precision)
            del os.environ["CRA_PREDICT_ZERO_COPY"]
            pcie_zc_2, _ = pcie_rate([net_e, net_f])
            net_e.close()
            net_f.close()
            net_b.close()
            # predict() on pinned buffers: zero-copy when nothing else is in flight on the device, staged through the DMA engines when
            # another user's forward is (rise_net.hip: RiseNet::submit) -- `zero_copy_*` say which form the last call of each leg took
            pcie = {"one_net_evals_per_sec": round(pcie_rate_1, 1), "two_nets_in_flight_evals_per_sec": round(pcie_rate_2, 1),
                    "zero_copy_one_net": bool(zc1), "zero_copy_two_nets": bool(zc2), "copy_path_one_net_evals_per_sec": round(pcie_copy_1, 1),
                    "copy_path_two_nets_evals_per_sec": round(pcie_copy_2, 1),
                    "zero_copy_forced_two_nets_evals_per_sec": round(pcie_zc_2, 1), "iterations": it,
                    "bytes_per_batch": {"planes_in": args.batch * cfg.nb_input_channels * 256, "probs_out": args.batch * cfg.nb_policy * 4,
                                        "value_out": args.batch * 4},
                    "fraction_of_value_one_net": round(pcie_rate_1 / value, 4),
                    "fraction_of_value_two_nets": round(pcie_rate_2 / value, 4)}
        full = {
            "metric": "nn_evals_per_sec", "value": round(value, 1), "value_precision": args.precision, "unit": "evals/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"float16": "f16", "float16x3": "f16x3", "float16p8": "f16x3+e5m2", "float32": "f32"}[args.precision], "data": "synthetic",
            "config": {"workload": f"crazyhouse RISEv2 {args.blocks}-block (34x8x8 planes -> 5184 policy + value), "
                                   f"batch={args.batch}, inputs resident in HBM, random-init seeded weights",
                       "batch": args.batch, "parallelism": f"replicas x{world}" + (" (dry ranks: one GPU, rehearsal of the launch)" if args.dry_ranks else ""),
                       "collective_backend": collective_backend, "precision": args.precision,
                       "flops_per_position": net.flops_per_position()},
            "timed_region": {"repeats": len(regions), "steps_per_repeat": args.steps, "seconds_total": round(float(sum(regions)), 4),
                             "ms_per_step_median": round(elapsed / args.steps * 1e3, 4),
                             "ms_per_step_min": round(min(regions) / args.steps * 1e3, 4),
                             "ms_per_step_max": round(max(regions) / args.steps * 1e3, 4)},
            "roofline": roofline,
        }
        if args.full and not args.no_cpu_baseline and world == 1:        # (rank 0 at N = 1 only: the other ranks of a node would wait for it)
            full["cpu_baseline"] = cpu_baseline(cfg, sd, x)
        if pcie is not None:
            # SURVEY 8(d) Metric 1 is CrazyAra's `inference` loop INCLUDING the host copies (crazyara.cpp:156-181): one blocking user
            full["pcie_inclusive"] = pcie
        full["modes"] = modes
        if nn_by_batch:
            full["nn_by_batch"] = nn_by_batch
        if dropin is not None:
            full["dropin_reference_search"] = dropin
        if mcts_configs:
            full["mcts_configs"] = mcts_configs
        if game_configs:
            full["game_configs"] = game_configs
        if mcts:
            full["mcts"] = mcts
        if mcts_headline_mode:
            full["mcts_other_mode"] = mcts_headline_mode
        full["bench_seconds"] = round(time.perf_counter() - t_bench_start, 1)
        out = compact_record(full, args.detail_out)
        try:
            with open(args.detail_out, "w") as f:
                json.dump(full, f, indent=1)
        except OSError as e:
            out["detail"] = f"not written: {e}"
    net.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        record_out.write(json.dumps(out) + "\n")
        record_out.flush()


if __name__ == "__main__":
    main()
