"""Writes tests/golden/nn_alphavile-{tiny,normal,normal-wdlp}.npz: inputs and outputs of the reference's own AlphaVile module.

The module is get_alpha_vile_model (DeepCrazyhouse/src/domain/neural_net/architectures/pytorch/alpha_vile.py) with the seeded weights of
crazyara_amd.rise_config.make_state_dict loaded by load_state_dict(strict=True) -- which pins the parameter names the exporter and the
C++ reader rely on.  Batch 4, chess v3.0 planes (tests/alphavile_oracle.py: CASES).  Needs the reference checkout (REFERENCE_ROOT,
default /root/reference); the GPU tests only read the .npz files.

    python scripts/make_alphavile_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import alphavile_oracle as ao  # noqa: E402


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, (size, _, _) in ao.CASES.items():
        cfg, sd, x = ao.make_case(name)
        m = ao.reference_alpha_vile(size, cfg)
        m.load_state_dict(sd, strict=True)
        with torch.no_grad():
            out = m(x)
        value, logits = out[0], out[1]
        arrays = dict(x=x.numpy().astype(np.float32), value=value.numpy().reshape(-1).astype(np.float32),
                      logits=logits.numpy().astype(np.float32))
        if cfg.use_wdl and cfg.use_plys_to_end:
            arrays["aux"] = out[2].numpy().astype(np.float32)     # cat(wdl logits, plys), process_value_policy_head
        path = os.path.join(out_dir, f"nn_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(path, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
