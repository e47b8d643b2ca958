"""The expert sets added kernels and changed none: every gfx950 kernel the library had before them has the same symbol, instruction
count and instruction text as in the listing made from the commit before (tests/golden/isa_kernels_before_experts.json, written by
scripts/isa_kernel_counts.py), and the only new kernels are the four indexed first / last kernels of a routed batch.  hipcc -S, no GPU.

This pins the library's kernels to ONE earlier commit, which is what the change that added the expert sets had to show.  A later change
that touches a kernel on purpose makes the record anew from the commit it starts from and lists its own new kernels in NEW_KERNELS:

    for f in <every .hip under crazyara_amd/csrc of that commit>; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC <build.device_flags()> -x hip --cuda-device-only -S $f -o <its file name>.s; done
    python scripts/isa_kernel_counts.py *.s > tests/golden/isa_kernels_before_experts.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("planes_from_desc_indexed_kernel", "gather_probs_indexed_kernel", "scatter_rows_indexed_kernel", "gather_planes_indexed_kernel")


def test_existing_kernels_are_unchanged_and_only_the_indexed_kernels_are_new(tmp_path):
    from crazyara_amd import build
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_kernel_counts
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_kernels_before_experts.json")))
    procs = []
    for src in build.sources():
        if not src.endswith(".hip"):
            continue
        out = tmp_path / (os.path.basename(src) + ".s")
        cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *build.device_flags(), "-x", "hip", "--cuda-device-only", "-S",
               src, "-o", str(out)]
        procs.append((out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path))))
    now = {}
    for out, p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, log
        now[out.name] = isa_kernel_counts.kernel_counts(str(out))
    assert set(before) <= set(now), set(before) - set(now)
    assert sum(len(v) for v in before.values()) >= 90
    added = []
    for listing, kernels in now.items():
        old = before.get(listing, {})
        for sym, (count, digest) in old.items():
            assert sym in kernels, f"{listing}: {sym} is gone"
            assert kernels[sym][0] == count, f"{listing}: {sym} has {kernels[sym][0]} instructions, had {count}"
            assert kernels[sym][1] == digest, f"{listing}: the instructions of {sym} changed"
        added += [s for s in kernels if s not in old]
    assert len(added) == len(NEW_KERNELS), added
    for name in NEW_KERNELS:
        assert any(name in s for s in added), (name, added)
