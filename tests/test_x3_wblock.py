"""The one-launch bottleneck block at trunk widths 128 / 192 / 224 (csrc/nn/x3_wblock.cpp, precision suffix "-wblock"), without a GPU:
the compiled kernels' resources from the gfx950 listing (hipcc -S) and the refusals that come before a device is touched.

Every block_x3w_kernel<C, KS> must keep its state in registers (0 bytes of scratch) and its tiles within the CU's 160 KiB of LDS; the
dynamic LDS size is restated here from the kernel's documented map -- xh / xl [64][C + 16] halves, the t2 pair in two buffers of
[64][128 + 16] halves, the eight waves' depthwise records (1 KiB per wave for 3x3, 2 KiB for 5x5)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "crazyara_amd", "csrc", "nn", "x3_wblock.cpp")
WIDTHS = (128, 192, 224)
KERNEL_SIZES = (3, 5)
LDS_LIMIT = 160 * 1024


def dynamic_lds_bytes(C, ks):
    return (2 * 64 * (C + 16) + 4 * 64 * (128 + 16)) * 2 + 8 * (1024 if ks == 3 else 2048)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from crazyara_amd import build
    out = tmp_path_factory.mktemp("x3_wblock") / "x3_wblock.s"
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *build.device_flags(), "-x", "hip", "--cuda-device-only", "-S",
           SRC, "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout
    return str(out)


def kernel_metadata(listing):
    """symbol -> {key: int} from the listing's amdhsa.kernels metadata"""
    text = open(listing).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, flags=re.M)}
    return kernels


def test_all_six_instantiations_exist_without_scratch_and_within_the_lds(listing):
    kernels = kernel_metadata(listing)
    for C in WIDTHS:
        for ks in KERNEL_SIZES:
            sym = [s for s in kernels if f"block_x3w_kernelILi{C}ELi{ks}EE" in s]
            assert len(sym) == 1, (C, ks, sorted(kernels))
            m = kernels[sym[0]]
            print(f"block_x3w_kernel<{C}, {ks}>: {m['vgpr_count']} VGPRs (+ {m.get('agpr_count', 0)} AGPRs), {m['sgpr_count']} SGPRs, "
                  f"scratch {m['private_segment_fixed_size']} B, LDS {m['group_segment_fixed_size']} + {dynamic_lds_bytes(C, ks)} B")
            assert m["private_segment_fixed_size"] == 0, (C, ks, m)
            assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (C, ks, m)
            assert m["group_segment_fixed_size"] + dynamic_lds_bytes(C, ks) <= LDS_LIMIT, (C, ks, m)
            assert m["max_flat_workgroup_size"] == 512
    assert sum("block_x3w_kernel" in s for s in kernels) == len(WIDTHS) * len(KERNEL_SIZES)


def test_the_listing_has_no_packed_f32_and_no_reader_in_the_shadow_of_an_mfma(listing):
    """what tests/test_isa_hazards.py asks of the .hip listings, asked of this file's"""
    packed = [l.strip() for l in open(listing) if l.strip().startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))]
    assert not packed, packed[:5]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_mfma_hazards.py"), listing], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "total 0", r.stdout[-3000:]
    assert sum(1 for l in lines if "block_x3w_kernel" in l and l.endswith("0 short distances")) == 6


@pytest.mark.parametrize("precision", ["float32-wblock", "float16-wblock", "fp8-wblock", "int8-wblock"])
def test_wblock_on_another_precision_is_refused_by_message(hip_lib, tmp_path, precision):
    """parsed before the model directory is read or a device is touched"""
    from crazyara_amd import _capi
    lib = _capi.load()
    assert not lib.mi_net_create(str(tmp_path).encode(), 0, 4, precision.encode())
    assert "`-wblock` is a float16x3 kernel family" in _capi.last_error() and precision in _capi.last_error()


def test_an_expert_set_refuses_the_suffix_by_name(hip_lib, tmp_path):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    for prec in (b"float16x3-wblock", b"float16p8-wblock"):
        assert not lib.mi_net_create_experts(root.encode(), 0, 8, prec, ec.LICHESS)
        assert "float16x3" in _capi.last_error() and prec.decode() in _capi.last_error()
