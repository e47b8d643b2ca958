"""GPU: precision "float16x3-wblock" -- the mobile-bottleneck blocks of 128 / 192 / 224-channel nets in one launch each
(csrc/nn/x3_wblock.cpp: block_x3w_kernel<C, KS>) instead of three layer launches.

Held to the float16x3 bounds of tests/test_alphavile_gpu.py (TOL["float16x3"]: logits 1e-4, value 1e-4, probabilities 1e-6, aux 1e-4)
against the fp32 restatement and, where one exists, the golden.  Against plain float16x3 on the same net and inputs the logits stay
within LAYER_PATH_BOUND = 2e-5: the two forms compute the same products and differ in the order of their f32 sums only (DESIGN 2's bound
for two float16x3 forms of one net).  Measured on the MI355X: see the table in profiles/NOTES.md, "AlphaVile: one-launch blocks".

The nets: a plain 224-channel net (C_op 448 / 320 / 448: full chunks and a 64-channel tail, 3x3 and 5x5, an eca_se gate fed by the block
before it), a block between two transformer blocks, an eca_se block right behind a transformer block (its squeeze comes from an SE launch),
the 192 / 128-channel nets of test_other_trunk_widths_run_on_the_layer_kernels (C_op 64 / 96 / 128: less than a chunk, ca_se and eca_se
gates on the input) and AlphaVile-tiny with its golden."""
import numpy as np
import pytest
import torch

import alphavile_oracle as ao
import nn_cases
from crazyara_amd import rise_config as rc
from oracle import rise_oracle as ro
from test_alphavile_gpu import REDUCED, TOL, logit_tol

pytestmark = pytest.mark.gpu

LAYER_PATH_BOUND = 2e-5
NETS = ("plain-224", "ntb-224-first-last", "ntb-128-eca", "mobile-192", "mobile-128", "alphavile-tiny")


def mobile(channels):
    """the "mobile" net of tests/test_nn_parity_gpu.py::test_other_trunk_widths_run_on_the_layer_kernels"""
    cfg = ro.rise_v2_config(3, 34, 81)
    cfg.se_types = [None, "ca_se", "eca_se"]
    cfg.kernels = [3, 5, 3]
    cfg.channels_operating_init, cfg.channel_expansion = 64, 32
    cfg.channels = channels
    cfg.name = f"mobile-{channels}"
    return cfg


_cases = {}


def case(name):
    """(cfg, state dict, planes, input version, restatement, golden or None), made once"""
    if name in _cases:
        return _cases[name]
    golden = None
    if name in REDUCED:
        factory, seed = REDUCED[name]
        cfg = factory()
        sd = rc.make_state_dict(cfg, seed=seed)
        if not cfg.has_transformers:
            sd["policy_head.body.3.weight"] = sd["policy_head.body.3.weight"] * 0.5
        x, version, forward = nn_cases.synthetic_planes(5, 52, seed), "3.0", ao.forward
    elif name.startswith("mobile-"):
        cfg = mobile(int(name.split("-")[1]))
        sd = ro.make_state_dict(cfg, seed=90 + cfg.channels)
        x, version, forward = nn_cases.synthetic_planes(5, 34, 17), "1.0", ro.forward
    else:
        cfg, sd, x = ao.make_case(name)
        golden = np.load(nn_cases.GOLDEN_DIR + f"/nn_{name}.npz")
        np.testing.assert_array_equal(golden["x"], x.numpy())
        version, forward = "3.0", ao.forward
    _cases[name] = (cfg, sd, x, version, forward, golden)
    return _cases[name]


def restatement(name, x=None):
    cfg, sd, x0, _, forward, _ = case(name)
    o_value, o_logits, o_aux = forward(cfg, sd, x0 if x is None else x)
    return o_value.numpy().reshape(-1), o_logits.numpy(), None if o_aux is None else o_aux.numpy()


_refs = {}


def reference(name):
    if name not in _refs:
        _refs[name] = restatement(name)
    return _refs[name]


def predict(tmp_path, name, precision, x=None):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, x0, version, _, _ = case(name)
    x = x0 if x is None else x
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version=version)
    B = x.shape[0]
    net = HipAPI(0, B, d, precision, keep_logits=True)
    value = np.full(B, 7.0, np.float32)
    probs = np.full(B * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(B * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(np.ascontiguousarray(x.numpy()), value, probs, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy()
    net.close()
    return value, probs.reshape(B, -1), aux, logits


_runs = {}


def cached_predict(tmp_path, name, precision):
    if (name, precision) not in _runs:
        _runs[(name, precision)] = predict(tmp_path, name, precision)
    return _runs[(name, precision)]


def check(ref, value, probs, aux, logits, golden=None):
    tol = TOL["float16x3"]
    refs = [ref]
    if golden is not None:
        refs.append((golden["value"], golden["logits"], golden["aux"] if "aux" in golden else None))
    for ref_v, ref_l, ref_a in refs:
        print(f"value {np.abs(value - ref_v).max():.2e}  logits {np.abs(logits - ref_l).max():.2e}")
        assert np.abs(value - ref_v).max() < tol["value"]
        assert np.abs(logits - ref_l).max() < logit_tol(tol, ref_l)
        if ref_a is not None:
            assert np.abs(aux.reshape(-1, 4) - ref_a).max() < tol["aux"]
    p = torch.softmax(torch.from_numpy(ref[1]), dim=1).numpy()
    print(f"probabilities {np.abs(probs - p).max():.2e}")
    assert np.abs(probs - p).max() < tol["prob"]


@pytest.mark.parametrize("name", NETS)
def test_predict_matches_the_restatement_and_the_golden(tmp_path, hip_lib, name):
    check(reference(name), *cached_predict(tmp_path, name, "float16x3-wblock"), golden=case(name)[5])


@pytest.mark.parametrize("name", NETS)
def test_logits_stay_within_the_bound_of_two_float16x3_forms(tmp_path, hip_lib, name):
    """float16x3 on the layer kernels and float16x3-wblock: the same products in another f32 summation order"""
    layer = cached_predict(tmp_path, name, "float16x3")
    fused = cached_predict(tmp_path, name, "float16x3-wblock")
    ref_l = reference(name)[1]
    d = float(np.abs(layer[3] - fused[3]).max())
    print(f"{name}: max |logits(float16x3-wblock) - logits(float16x3)| = {d:.3e}; against the restatement: layer path "
          f"{np.abs(layer[3] - ref_l).max():.3e}, wblock {np.abs(fused[3] - ref_l).max():.3e}; value {np.abs(layer[0] - fused[0]).max():.3e}")
    assert d < LAYER_PATH_BOUND
    assert np.abs(layer[0] - fused[0]).max() < LAYER_PATH_BOUND


@pytest.mark.parametrize("batch", [1, 5, 256])
def test_batch_sizes(tmp_path, hip_lib, batch):
    x = nn_cases.synthetic_planes(batch, 52, 500 + batch)
    check(restatement("alphavile-tiny", x), *predict(tmp_path, "alphavile-tiny", "float16x3-wblock", x))


@pytest.mark.parametrize("name", ["ntb-224-first-last", "alphavile-normal"])
def test_op_list_has_one_launch_per_block_and_one_attention_launch_per_ntb(tmp_path, hip_lib, name):
    from crazyara_amd.neuralnetapi import HipAPI
    if name in REDUCED:
        cfg, sd, _, _, _, _ = case(name)
    else:
        cfg, sd, _ = ao.make_case(name)
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version="3.0")
    net = HipAPI(0, 4, d, "float16x3-wblock")
    names = [n for n, _ in net.time_ops(1)]
    net.close()
    ntbs = sum(bool(cfg.transformer(i)) for i in range(len(cfg.kernels)))
    assert ntbs >= 2
    assert names.count("block_x3w") == len(cfg.kernels) - ntbs
    assert "depthwise" not in names
    assert names.count("attention") == ntbs
    assert not {"tower", "tower_x3", "fused_block", "block_x3", "head", "forward", "stem"} & set(names)


def test_two_runs_and_poisoned_lds_give_identical_bits(tmp_path, hip_lib, lds_poison):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    batch = 9
    x = nn_cases.synthetic_planes(batch, 52, 77).numpy().reshape(-1)
    net = HipAPI(0, batch, d, "float16x3-wblock")
    outs = []
    for pattern in (0x00000000, 0x00000000, 0xffffffff, 0x7f7f7f7f, 0x7bff7bff, 0x7f800000):
        assert lds_poison.poison_lds(pattern, pattern, 0, 0) == 0
        v = np.zeros(batch, np.float32)
        p = np.zeros(batch * cfg.nb_policy, np.float32)
        net.predict(x, v, p)
        outs.append((v, p))
    net.close()
    assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all()
    for v, p in outs[1:]:
        assert np.array_equal(v, outs[0][0]) and np.array_equal(p, outs[0][1])


def test_float16p8_wblock_gives_the_bits_of_float16x3_wblock(tmp_path, hip_lib):
    a = cached_predict(tmp_path, "alphavile-tiny", "float16x3-wblock")
    b = predict(tmp_path, "alphavile-tiny", "float16p8-wblock")
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


@pytest.mark.parametrize("precision", ["float32-wblock", "float16-wblock", "fp8-wblock", "int8-wblock"])
def test_wblock_on_another_precision_is_refused(tmp_path, hip_lib, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    with pytest.raises(Exception, match="`-wblock` is a float16x3 kernel family"):
        HipAPI(0, 4, d, precision)


def _unqualified(kind):
    if kind == "256-wide":
        cfg, sd, _ = nn_cases.make_case("risev2-3")
        assert cfg.channels == 256
        return cfg, sd
    if kind == "mobile-512":
        cfg = mobile(512)
    elif kind == "a0-128":
        cfg = ro.alpha_zero_config(2, 34, 81, 4)
        cfg.channels = cfg.channels_operating_init = 128
        cfg.name = "a0-128"
    else:
        cfg = ro.rise_classical_config(2, 34, 81)
        cfg.channels = cfg.channels_operating_init = 192
        cfg.name = "classical-192"
    return cfg, ro.make_state_dict(cfg, seed=7)


@pytest.mark.parametrize("precision", ["float16x3-wblock", "float16p8-wblock"])
@pytest.mark.parametrize("kind", ["256-wide", "mobile-512", "a0-128", "classical-192"])
def test_wblock_on_a_net_without_a_qualifying_block_is_refused(tmp_path, hip_lib, kind, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd = _unqualified(kind)
    d = nn_cases.export_case(tmp_path, kind, cfg, sd)
    with pytest.raises(Exception, match="no block of this model qualifies"):
        HipAPI(0, 4, d, precision)
    if precision == "float16x3-wblock":
        HipAPI(0, 4, d, "float16x3").close()                       # (the same directory loads without the suffix)


@pytest.mark.parametrize("precision", ["float16x3-wblock", "float16p8-wblock"])
def test_an_expert_set_refuses_the_suffix(tmp_path, hip_lib, precision):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    assert not lib.mi_net_create_experts(root.encode(), 0, 8, precision.encode(), ec.LICHESS)
    assert "an expert set runs Precision float16x3" in _capi.last_error() and precision in _capi.last_error()
