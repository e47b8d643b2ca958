"""Runs of consecutive bottleneck blocks in one launch at trunk widths 128 / 192 / 224 (csrc/nn/x3_wtower.cpp, precision suffix
"-wtower"), without a GPU: the compiled kernels' resources from the gfx950 listing (hipcc -S) and the refusals that come before a device
is touched.

Every tower_x3w_kernel<C> must keep its state in registers (0 bytes of scratch, at most 256 VGPRs + AGPRs) and its tiles within the CU's
160 KiB of LDS.  Its LDS map is block_x3w_kernel's with the waves' record areas sized for a 5x5 depthwise, whatever the blocks of the run:
the dynamic size is tests/test_x3_wblock.py's restatement at ks = 5."""
import os
import subprocess
import sys

import pytest

from test_x3_wblock import LDS_LIMIT, WIDTHS, dynamic_lds_bytes, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "crazyara_amd", "csrc", "nn", "x3_wtower.cpp")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from crazyara_amd import build
    out = tmp_path_factory.mktemp("x3_wtower") / "x3_wtower.s"
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *build.device_flags(), "-x", "hip", "--cuda-device-only", "-S",
           SRC, "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout
    return str(out)


def test_all_three_instantiations_exist_without_scratch_within_256_registers_and_the_lds(listing):
    kernels = kernel_metadata(listing)
    for C in WIDTHS:
        sym = [s for s in kernels if f"tower_x3w_kernelILi{C}EE" in s]
        assert len(sym) == 1, (C, sorted(kernels))
        m = kernels[sym[0]]
        print(f"tower_x3w_kernel<{C}>: {m['vgpr_count']} VGPRs (+ {m.get('agpr_count', 0)} AGPRs), {m['sgpr_count']} SGPRs, "
              f"scratch {m['private_segment_fixed_size']} B, LDS {m['group_segment_fixed_size']} + {dynamic_lds_bytes(C, 5)} B")
        assert m["private_segment_fixed_size"] == 0, (C, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (C, m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= 256, (C, m)
        assert m["group_segment_fixed_size"] + dynamic_lds_bytes(C, 5) <= LDS_LIMIT, (C, m)
        assert m["max_flat_workgroup_size"] == 512
    assert sum("tower_x3w_kernel" in s for s in kernels) == len(WIDTHS)


def test_the_listing_has_no_packed_f32_and_no_reader_in_the_shadow_of_an_mfma(listing):
    """what tests/test_x3_wblock.py asks of x3_wblock.cpp's listing, asked of this file's"""
    packed = [l.strip() for l in open(listing) if l.strip().startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))]
    assert not packed, packed[:5]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_mfma_hazards.py"), listing], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "total 0", r.stdout[-3000:]
    assert sum(1 for l in lines if "tower_x3w_kernel" in l and l.endswith("0 short distances")) == 3


def _refused(tmp_path, precision):
    from crazyara_amd import _capi
    lib = _capi.load()
    assert not lib.mi_net_create(str(tmp_path).encode(), 0, 4, precision.encode())
    err = _capi.last_error()
    assert precision in err, err
    return err


@pytest.mark.parametrize("precision", ["float32-wtower", "float16-wtower", "fp8-wtower", "int8-wtower"])
def test_wtower_on_another_precision_is_refused_by_message(hip_lib, tmp_path, precision):
    """parsed before the model directory is read or a device is touched"""
    assert "`-wtower` is a float16x3 kernel family (float16x3-wtower | float16p8-wtower)" in _refused(tmp_path, precision)


@pytest.mark.parametrize("precision", ["float16x3-unfused-wtower", "float16p8-unfused-wtower"])
def test_wtower_with_unfused_is_refused(hip_lib, tmp_path, precision):
    assert "`-wtower` and `-unfused` exclude each other" in _refused(tmp_path, precision)


@pytest.mark.parametrize("precision", ["float16x3-wtower-wsplit", "float16x3-wsplit-wtower", "float16x3-wtower-wnet"])
def test_one_suffix_of_the_chain_at_a_time(hip_lib, tmp_path, precision):
    assert "unsupported precision" in _refused(tmp_path, precision)


def test_the_suffixes_parse(hip_lib, tmp_path):
    """(an empty directory: the precisions that exist get as far as the missing model file)"""
    from crazyara_amd import _capi
    lib = _capi.load()
    for precision in ("float16x3-wtower", "float16p8-wtower", "float16x3-wsplit", "float16p8-wsplit", "float16x3-wnet", "float16x3-wblock", "float16x3"):
        assert not lib.mi_net_create(str(tmp_path).encode(), 0, 4, precision.encode())
        err = _capi.last_error()
        assert "kernel family" not in err and "exclude each other" not in err and "unsupported precision" not in err, (precision, err)


def test_an_expert_set_refuses_the_suffix_by_name(hip_lib, tmp_path):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    for prec in (b"float16x3-wtower", b"float16p8-wtower"):
        assert not lib.mi_net_create_experts(root.encode(), 0, 8, prec, ec.LICHESS)
        assert "an expert set runs Precision float16x3" in _capi.last_error() and prec.decode() in _capi.last_error()
