"""AlphaVile throughput: evals/s of predict-sized forwards (graph replays) at batch 256 for the four sizes in float16x3, float16 and
float32, and time_ops per op so that the attention launch's share of the forward is visible.  Seeded weights (the timing does not depend
on them).  One JSON line per (size, precision) on stdout; --ops also prints the per-op table.

    python scripts/alphavile_bench.py [--batch 256] [--iters 50] [--sizes tiny,small,normal,large] [--precisions float16x3,float16,float32] [--ops]

A/B of the one-launch blocks: --precisions float16x3,float16x3-wblock,float16x3,float16x3-wblock,... (a precision may repeat: the runs of a
size then interleave in one process); of the one-launch transformer blocks: float16x3-wblock,float16x3-wnet,...  ntb_ms is the time of a
net's transformer blocks: the ntb_x3w ops, or the nine layer ops of every attention launch (four before it, four behind).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from crazyara_amd import netfile, rise_config as rc  # noqa: E402
from crazyara_amd.neuralnetapi import HipAPI  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sizes", default="tiny,small,normal,large")
    ap.add_argument("--precisions", default="float16x3,float16,float32")
    ap.add_argument("--ops", action="store_true")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="alphavile_bench_")
    B = args.batch
    rng = np.random.default_rng(0)
    for size in args.sizes.split(","):
        cfg = rc.alpha_vile_config(size)
        d = os.path.join(tmp, size)
        netfile.export_rise(os.path.join(d, f"alphavile-{size}-v3.0.cranet"), cfg, rc.make_state_dict(cfg, seed=1), input_version="3.0")
        x = (rng.random((B, cfg.nb_input_channels, 8, 8)) < 0.1).astype(np.float32)
        for prec in args.precisions.split(","):
            net = HipAPI(0, B, d, prec)
            value = np.zeros(B, np.float32)
            probs = np.zeros(B * cfg.nb_policy, np.float32)
            for _ in range(5):
                net.predict(x, value, probs)
            ms = net.time_forward(args.iters) / args.iters if hasattr(net, "time_forward") else None
            t0 = time.perf_counter()
            for _ in range(args.iters):
                net.predict(x, value, probs)
            predict_ms = (time.perf_counter() - t0) * 1e3 / args.iters
            ops = net.time_ops(max(1, args.iters // 5))
            total = sum(t for _, t in ops)
            att = sum(t for n, t in ops if n == "attention")
            names = [n for n, _ in ops]
            ntb = sum(t for n, t in ops if n == "ntb_x3w") + sum(sum(t for _, t in ops[i - 2:i + 7]) for i, n in enumerate(names) if n == "attention")
            rec = dict(net=f"alphavile-{size}", precision=prec, batch=B, forward_ms=ms, predict_ms=round(predict_ms, 4),
                       evals_per_s=round(B / ((ms if ms else predict_ms) * 1e-3)), launches=len(ops),
                       ops_ms_sum=round(total, 4), attention_ms=round(att, 4), attention_share=round(att / total, 4), ntb_ms=round(ntb, 4),
                       mflop_per_board=round(net.flops_per_position() / 1e6, 1))
            print(json.dumps(rec), flush=True)
            if args.ops:
                for i, (n, t) in enumerate(ops):
                    print(f"  {i:3d} {n:20s} {t * 1e3:8.1f} us")
            net.close()


if __name__ == "__main__":
    main()
