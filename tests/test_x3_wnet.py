"""The one-launch NextViT transformer block (csrc/nn/x3_wntb.cpp, precision suffix "-wnet"), without a GPU: the compiled kernels'
resources from the gfx950 listing (hipcc -S) and the refusals that come before a device is touched.

Every ntb_x3w_kernel<C> must keep its state in registers (0 bytes of scratch) and its tiles within the CU's 160 KiB of LDS; the dynamic
LDS size is restated here from the kernel's documented map -- xs f32 [64][C + 4], the operand pair [65][C + 16] halves, and the stage
region: one head's q | k | v f32 [64][100] with its output pair [64][40] halves, or a chunk's t2 pair [64][128 + 16] halves."""
import os
import subprocess
import sys

import pytest

from test_x3_wblock import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "crazyara_amd", "csrc", "nn", "x3_wntb.cpp")
WIDTHS = (128, 192, 224)
LDS_LIMIT = 160 * 1024


def dynamic_lds_bytes(C):
    xs = 64 * (C + 4) * 4
    operands = 2 * 65 * (C + 16) * 2
    head = 64 * 100 * 4 + 2 * 64 * 40 * 2
    t2 = 2 * 64 * (128 + 16) * 2
    return xs + operands + max(head, t2)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from crazyara_amd import build
    out = tmp_path_factory.mktemp("x3_wntb") / "x3_wntb.s"
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *build.device_flags(), "-x", "hip", "--cuda-device-only", "-S",
           SRC, "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout
    return str(out)


def test_all_three_instantiations_exist_without_scratch_and_within_the_lds(listing):
    kernels = kernel_metadata(listing)
    for C in WIDTHS:
        sym = [s for s in kernels if f"ntb_x3w_kernelILi{C}EE" in s]
        assert len(sym) == 1, (C, sorted(kernels))
        m = kernels[sym[0]]
        print(f"ntb_x3w_kernel<{C}>: {m['vgpr_count']} VGPRs (+ {m.get('agpr_count', 0)} AGPRs), {m['sgpr_count']} SGPRs, "
              f"scratch {m['private_segment_fixed_size']} B, LDS {m['group_segment_fixed_size']} + {dynamic_lds_bytes(C)} B")
        assert m["private_segment_fixed_size"] == 0, (C, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (C, m)
        assert m["group_segment_fixed_size"] + dynamic_lds_bytes(C) <= LDS_LIMIT, (C, m)
        assert m["max_flat_workgroup_size"] == 512
    assert sum("ntb_x3w_kernel" in s for s in kernels) == len(WIDTHS)


def test_the_listing_has_no_packed_f32_and_no_reader_in_the_shadow_of_an_mfma(listing):
    """what tests/test_isa_hazards.py asks of the .hip listings, asked of this file's"""
    packed = [l.strip() for l in open(listing) if l.strip().startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))]
    assert not packed, packed[:5]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_mfma_hazards.py"), listing], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "total 0", r.stdout[-3000:]
    assert sum(1 for l in lines if "ntb_x3w_kernel" in l and l.endswith("0 short distances")) == len(WIDTHS)


@pytest.mark.parametrize("precision", ["float32-wnet", "float16-wnet", "fp8-wnet", "int8-wnet"])
def test_wnet_on_another_precision_is_refused_by_message(hip_lib, tmp_path, precision):
    """parsed before the model directory is read or a device is touched"""
    from crazyara_amd import _capi
    lib = _capi.load()
    assert not lib.mi_net_create(str(tmp_path).encode(), 0, 4, precision.encode())
    assert "`-wnet` is a float16x3 kernel family" in _capi.last_error() and precision in _capi.last_error()


@pytest.mark.parametrize("precision", ["float16x3-wnet-unfused", "float16x3-unfused-wnet", "float16p8-unfused-wnet"])
def test_wnet_with_unfused_is_refused(hip_lib, tmp_path, precision):
    from crazyara_amd import _capi
    lib = _capi.load()
    assert not lib.mi_net_create(str(tmp_path).encode(), 0, 4, precision.encode())
    err = _capi.last_error()
    assert precision in err and ("`-wnet` and `-unfused` exclude each other" in err or "unsupported precision" in err), err


def test_an_expert_set_refuses_the_suffix_by_name(hip_lib, tmp_path):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    for prec in (b"float16x3-wnet", b"float16p8-wnet"):
        assert not lib.mi_net_create_experts(root.encode(), 0, 8, prec, ec.LICHESS)
        assert "float16x3" in _capi.last_error() and prec.decode() in _capi.last_error()
