"""Which precision modes can be held to their parity bounds on trained-net-like weights (tests/nn_cases.trained_like)?

For every case of nn_cases.TRAINED_LIKE: the float64 oracle, the fp32 oracle and, per mode, that mode's CPU emulation where one exists
for the case.  Written to tests/golden/trained_like_emulation.json: the emulation's error against float64, the bound of
tests/test_trained_like_gpu.py, and `eligible` -- the emulation is within HALF of the bound on logits, value and aux outputs.  The GPU
test runs a mode on the cases that are eligible for it and on no others.

    mode        emulation
    float32     the fp32 oracle (forward on the fp32 state dict)
    float16x3   oracle.rise_oracle.forward_x3 (NTB nets: none exists; the mode's design error is f32 round-off, the fp32 oracle stands in)
    float16p8   forward_p8
    float16     forward(sim_dtype=float16)
    fp8, int8   forward_fp8_tower / forward_int8_tower (calibrate_int8 on 64 synthetic_planes), bottleneck RISE nets only.  These two
                have no end-to-end bound: their tests hold every block to its own mode error, teacher-forced.  Their errors are recorded;
                eligible = the emulation's outputs are finite.

Run from the repository root:  python scripts/studies/trained_like_study.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nn_cases  # noqa: E402
from oracle import rise_oracle as ro  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "trained_like_emulation.json")
VALUE_BOUND = {"float32": 1e-4, "float16x3": 1e-4, "float16p8": 1e-4, "float16": 1e-3}


def logit_bound(mode, max_logit):
    if mode in ("float32", "float16x3"):
        return max(1e-4, 4e-5 * max_logit)
    return {"float16p8": 2.5e-4, "float16": 2.2e-3}[mode] * max_logit


def emulations(cfg, sd, x):
    """mode -> (value, logits, aux) of its emulation, for the modes that have one on this net"""
    out = {"float32": nn_cases.oracle_forward(cfg, sd, x)}
    if cfg.has_transformers:
        out["float16x3"] = out["float32"]
        return out
    out["float16x3"] = ro.forward_x3(cfg, sd, x)
    out["float16p8"] = ro.forward_p8(cfg, sd, x)
    out["float16"] = ro.forward(cfg, sd, x, sim_dtype=torch.float16)
    if not cfg.dense_blocks:
        out["fp8"] = ro.forward_fp8_tower(cfg, sd, x)
        calib = ro.calibrate_int8(cfg, sd, nn_cases.synthetic_planes(64, cfg.nb_input_channels, 555))
        out["int8"] = ro.forward_int8_tower(cfg, sd, x, calib)
    return out


def study(name):
    cfg, sd, x = nn_cases.trained_like_case(name)
    v64, l64, a64 = nn_cases.oracle_forward(cfg, ro.to_double(sd), x)
    max_logit = float(l64.abs().max())
    rec = dict(max_logit=max_logit, max_prob=float(torch.softmax(l64, 1).max()), max_abs_value=float(v64.abs().max()), modes={})
    for mode, (v, l, a) in emulations(cfg, sd, x).items():
        r = dict(logit_error=float((l.double() - l64).abs().max()), value_error=float((v.double() - v64).abs().max()))
        if a64 is not None:
            r["aux_error"] = float((a.double() - a64).abs().max())
        finite = bool(torch.isfinite(l).all() and torch.isfinite(v).all())
        if mode in VALUE_BOUND:
            r["logit_bound"], r["value_bound"] = logit_bound(mode, max_logit), VALUE_BOUND[mode]
            r["eligible"] = bool(finite and r["logit_error"] <= 0.5 * r["logit_bound"] and r["value_error"] <= 0.5 * r["value_bound"]
                                 and r.get("aux_error", 0.0) <= 0.5 * r["value_bound"]
                                 and (mode not in ("float32", "float16x3") or r["logit_bound"] < 1e-3))
        else:
            r["eligible"] = finite
        rec["modes"][mode] = r
        print(f"{name:22s} {mode:10s} " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()), flush=True)
    return rec


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    result = {name: study(name) for name in nn_cases.TRAINED_LIKE}
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
