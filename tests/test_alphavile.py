"""AlphaVile (RiseV3 with NextViT transformer blocks) on the host side: configs, seeded weights, the test-side restatement and the model
file's metadata -- against the reference's own module where /root/reference is present."""
import numpy as np
import pytest
import torch

import alphavile_oracle as ao
import nn_cases
from crazyara_amd import netfile, rise_config as rc
from oracle import rise_oracle as ro

SIZES = ["tiny", "small", "normal", "large"]


@pytest.mark.parametrize("size,channels,depth,ntbs,k5", [("tiny", 192, 15, [14], [1, 2, 6, 7, 8, 9, 10]),
                                                         ("small", 192, 22, [21], [0, 4, 5, 6, 10, 11, 13, 15, 17, 20]),
                                                         ("normal", 224, 26, [17, 25], None), ("large", 224, 37, [24, 36], None)])
def test_alpha_vile_config_shapes(size, channels, depth, ntbs, k5):
    cfg = rc.alpha_vile_config(size)
    assert cfg.channels == channels and len(cfg.kernels) == depth and cfg.channel_expansion == 0
    assert [i for i in range(depth) if cfg.transformer(i)] == ntbs
    if k5 is not None:
        assert [i for i, k in enumerate(cfg.kernels) if k == 5] == k5
    c5 = 256 if channels == 192 else 320
    assert cfg.channels_operating() == [c5 if k == 5 else 2 * channels for k in cfg.kernels]
    assert rc.ntb_widths(channels) == (160, channels - 160, 2 * channels)


def test_existing_configs_are_untouched():
    """The new fields default to off: C_op schedules and the exported header of the existing nets are as before."""
    cfg = rc.rise_v33_config()
    assert cfg.use_transformers is None and cfg.kernel_5_channel_ratio is None and not cfg.has_transformers
    assert cfg.channels_operating() == [224 + 32 * i - (32 * (i // 2) if k == 5 else 0) for i, k in enumerate(cfg.kernels)]


def test_export_read_round_trip_of_the_transformer_metadata(tmp_path):
    cfg = rc.alpha_vile_config("tiny")
    sd = rc.make_state_dict(cfg, seed=1)
    path = netfile.export_rise(str(tmp_path / "alphavile-tiny-v3.0.cranet"), cfg, sd, input_version="3.0")
    meta, tensors = netfile.read_cranet(path)
    assert meta["use_transformers"] == ",".join("1" if t else "0" for t in cfg.use_transformers)
    assert [int(c) for c in meta["channels_operating"].split(",")] == cfg.channels_operating()
    assert "body_spatial.15.e_mhsa.q.weight" in tensors and "body_spatial.15.mhca.group_conv3x3.weight" in tensors
    np.testing.assert_array_equal(tensors["body_spatial.15.mlp.conv1.bias"], sd["body_spatial.15.mlp.conv1.bias"].numpy())
    # a net without transformer blocks writes neither key
    cfg2 = rc.rise_v33_config()
    meta2, _ = netfile.read_cranet(netfile.export_rise(str(tmp_path / "r.cranet"), cfg2, rc.make_state_dict(cfg2, seed=1)))
    assert "use_transformers" not in meta2 and "channels_operating" not in meta2


@pytest.mark.parametrize("name", list(ao.CASES))
def test_attention_is_not_degenerate_on_the_seeded_nets(name):
    """Uniform attention weights move the outputs by far more than the GPU tolerances (1e-4 ... 4.8e-3): the tests see the softmax."""
    cfg, sd, x = ao.make_case(name)
    v, p, _ = ao.forward(cfg, sd, x)
    vu, pu, _ = ao.forward(cfg, sd, x, uniform_attention=True)
    assert float((v - vu).abs().max()) > 2e-2
    assert float((p - pu).abs().max()) > 0.5


def test_restatement_without_transformers_is_the_rise_oracle():
    cfg, sd, x = nn_cases.make_case("risev33-wdlp")
    for a, b in zip(ao.forward(cfg, sd, x), ro.forward(cfg, sd, x)):
        assert torch.allclose(a, b, atol=1e-5)


def test_flops_count_of_an_ntb():
    cfg = rc.alpha_vile_config("tiny")
    mf = ao.flops_per_position(cfg) / 1e6
    assert 300 < mf < 380          # ~340 MFLOP per board (the issue's estimate)


@pytest.mark.reference
@pytest.mark.parametrize("size", SIZES)
def test_state_dict_keys_and_shapes_equal_the_reference_module(has_reference, size):
    if not has_reference:
        pytest.skip("/root/reference not present (GPU box)")
    cfg = rc.alpha_vile_config(size)
    ref = ao.reference_alpha_vile(size, cfg).state_dict()
    sd = rc.make_state_dict(cfg, seed=2)
    assert set(ref) == set(sd)
    for k in ref:
        assert tuple(ref[k].shape) == tuple(sd[k].shape), k


@pytest.mark.reference
@pytest.mark.parametrize("name", ["alphavile-tiny", "alphavile-normal", "alphavile-normal-wdlp"])
def test_restatement_equals_the_reference_module(has_reference, name):
    if not has_reference:
        pytest.skip("/root/reference not present (GPU box)")
    cfg, sd, x = ao.make_case(name)
    m = ao.reference_alpha_vile(ao.CASES[name][0], cfg)
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        out = m(x)
    value, logits, aux = ao.forward(cfg, sd, x)
    assert float((out[0] - value).abs().max()) < 1e-5
    assert float((out[1] - logits).abs().max()) < 1e-5
    if aux is not None:
        assert float((out[2] - aux).abs().max()) < 1e-5


@pytest.mark.parametrize("name", list(ao.CASES))
def test_goldens_match_the_restatement(name):
    g = np.load(nn_cases.GOLDEN_DIR + f"/nn_{name}.npz")
    cfg, sd, x = ao.make_case(name)
    np.testing.assert_array_equal(g["x"], x.numpy())
    value, logits, aux = ao.forward(cfg, sd, x)
    assert np.abs(g["value"] - value.numpy().reshape(-1)).max() < 1e-5
    assert np.abs(g["logits"] - logits.numpy()).max() < 1e-5
    if aux is not None:
        assert np.abs(g["aux"] - aux.numpy()).max() < 1e-5


def test_the_attention_kernel_is_free_of_packed_f32_and_mfma_hazards(tmp_path):
    """tests/test_isa_hazards.py's two checks over attention.hip (that test's file list predates the kernel)."""
    import os
    import subprocess
    import sys
    from crazyara_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "attention.s"
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *build.device_flags(), "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(root, "crazyara_amd", "csrc", "nn", "attention.hip"), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout
    text = out.read_text()
    assert not [l for l in text.splitlines() if l.strip().startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))]
    assert text.count("v_mfma") >= 3
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "isa_mfma_hazards.py"), str(out)], stdout=subprocess.PIPE, text=True)
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "total 0" and sum(1 for l in lines if l.endswith("0 short distances")) == 3, r.stdout


def test_f16_storage_alone_exceeds_the_fused_nets_float16_bounds():
    """Why tests/test_alphavile_gpu.py does not hold float16 to test_nn_parity_gpu.py's float16 logit / aux bounds (2.2e-3 x max|logit|
    capped at 4.8e-3; 1e-3): the f16 roundings of the layer path, emulated on the fp32 forward with no kernel involved, already exceed
    them on the goldens (tiny: 9.0e-3 on the logits; normal-wdlp: 1.0e-3 on the aux outputs) -- and stay inside the bounds the GPU test uses (3.5e-3 x max|logit|, value 2e-3, aux 2e-3)."""
    for name in ao.CASES:
        cfg, sd, x = ao.make_case(name)
        value, logits, aux = ao.forward(cfg, sd, x)
        e_value, e_logits, e_aux = ao.forward_f16(cfg, sd, x)
        err, scale = float((e_logits - logits).abs().max()), float(logits.abs().max())
        assert err < min(1e-2, 3.5e-3 * scale)
        assert float((e_value - value).abs().max()) < 2e-3
        if aux is not None:
            assert float((e_aux - aux).abs().max()) < 2e-3
        if name == "alphavile-tiny":
            assert err > 4.8e-3                      # (9.0e-3: 2.3e-3 x max|logit|)
