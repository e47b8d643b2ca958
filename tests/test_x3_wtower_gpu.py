"""GPU: precision "float16x3-wtower" -- "-wnet", and every maximal run of two or more consecutive mobile-bottleneck blocks of a 128 /
192 / 224-channel net in one launch (csrc/nn/x3_wtower.cpp: tower_x3w_kernel<C>).  A gated block starts a run, a transformer block ends
one, a run of one block stays block_x3w_kernel's launch.

The run kernel is block_x3w_kernel's arithmetic block after block -- the same products, the same order of the f32 sums, the residual in
exact f32 -- so against "float16x3-wnet" on the same net and inputs every output is held to np.array_equal.  Against the fp32 restatement
(and AlphaVile-tiny's golden) the bounds are the float16x3 bounds of tests/test_alphavile_gpu.py (TOL["float16x3"]: logits 1e-4, value
1e-4, probabilities 1e-6, aux 1e-4).

The nets:
  plain-224            kernels [3, 5, 3], se [-, -, eca_se]: a run {0, 1} of a 3x3 and a 5x5 block with 64-channel tail chunks (C_op 448 /
                       320) whose last block leaves the channel sums; se_gate_w; a lone gated block_x3w
  run-224-gated-first  kernels [5, 3, 3, 5], se [-, eca_se, -, -]: block 0 stays a block_x3w and feeds the gate, run {1, 2, 3} has a gated
                       first block
  run-192-ntb          reduced(192, [3, 5, 5, 3, 3], ntbs = [2]): a run on either side of a transformer block, the tile dealing at 192
  run-128              reduced(128, [3, 3, 5, 3], ntbs = []): one project tile per wave, one run of four blocks
  alphavile-tiny       as shipped, with its golden: one run of 14 blocks in front of the transformer block"""
import numpy as np
import pytest

import alphavile_oracle as ao
import nn_cases
from crazyara_amd import rise_config as rc
from test_alphavile_gpu import reduced
from test_x3_wblock_gpu import _cases, _unqualified, cached_predict, case, check, predict, reference, restatement

pytestmark = pytest.mark.gpu

NETS = ("plain-224", "run-224-gated-first", "run-192-ntb", "run-128", "alphavile-tiny")


def _gated_first():
    return rc.RiseConfig(nb_input_channels=52, channels=224, channels_operating_init=448, channel_expansion=0, kernels=[5, 3, 3, 5],
                         se_types=[None, "eca_se", None, None], value_fc_size=224, channels_policy_head=76,
                         kernel_5_channel_ratio=0.7142857142857143, name="run-224-gated-first")


def _named(cfg, name):
    cfg.name = name
    return cfg


NEW = {
    "run-224-gated-first": (_gated_first, 45),
    "run-192-ntb": (lambda: _named(reduced(192, [3, 5, 5, 3, 3], [2]), "run-192-ntb"), 46),
    "run-128": (lambda: _named(reduced(128, [3, 3, 5, 3], []), "run-128"), 47),
}


def tcase(name):
    """tests/test_x3_wblock_gpu.py's case(), with this file's nets made the way it makes the reduced ones"""
    if name in NEW and name not in _cases:
        factory, seed = NEW[name]
        cfg = factory()
        sd = rc.make_state_dict(cfg, seed=seed)
        if not cfg.has_transformers:
            sd["policy_head.body.3.weight"] = sd["policy_head.body.3.weight"] * 0.5
        _cases[name] = (cfg, sd, nn_cases.synthetic_planes(5, 52, seed), "3.0", ao.forward, None)
    return case(name)


def test_the_nets_are_what_the_docstring_says():
    assert tcase("plain-224")[0].kernels == [3, 5, 3] and tcase("plain-224")[0].se_types == [None, None, "eca_se"]
    g = tcase("run-224-gated-first")[0]
    assert g.channels == 224 and g.kernels == [5, 3, 3, 5] and g.se_types == [None, "eca_se", None, None]
    n = tcase("run-192-ntb")[0]
    assert n.channels == 192 and [bool(n.transformer(i)) for i in range(5)] == [False, False, True, False, False]
    assert tcase("run-128")[0].channels == 128 and not tcase("run-128")[0].has_transformers
    assert tcase("plain-224")[2].shape[0] == 5 and tcase("alphavile-tiny")[2].shape[0] == 4


@pytest.mark.parametrize("name", NETS)
def test_wtower_gives_the_bits_of_wnet(tmp_path, hip_lib, name):
    """value, probabilities, aux and logits; the gated nets too: the squeeze is block_x3w_kernel's own epilogue code"""
    tcase(name)
    one = cached_predict(tmp_path, name, "float16x3-wnet")
    run = cached_predict(tmp_path, name, "float16x3-wtower")
    print(f"{name}: max |logits(float16x3-wtower) - logits(float16x3-wnet)| = {float(np.abs(one[3] - run[3]).max()):.3e}, "
          f"value {float(np.abs(one[0] - run[0]).max()):.3e}")
    assert np.isfinite(run[3]).all() and np.isfinite(run[0]).all()
    for u, v in zip(one, run):
        assert (u is None and v is None) or np.array_equal(u, v)


def test_float16p8_wtower_gives_the_bits_of_float16x3_wtower(tmp_path, hip_lib):
    a = cached_predict(tmp_path, "alphavile-tiny", "float16x3-wtower")
    b = predict(tmp_path, "alphavile-tiny", "float16p8-wtower")
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


@pytest.mark.parametrize("name", NETS)
def test_predict_matches_the_restatement_and_the_golden(tmp_path, hip_lib, name):
    tcase(name)
    check(reference(name), *cached_predict(tmp_path, name, "float16x3-wtower"), golden=case(name)[5])


def op_names(tmp_path, name, precision, batch=4):
    from crazyara_amd.neuralnetapi import HipAPI
    if name == "alphavile-normal":
        cfg, sd, _ = ao.make_case(name)
        version = "3.0"
    else:
        cfg, sd, _, version, _, _ = tcase(name)
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version=version)
    net = HipAPI(0, batch, d, precision)
    names = [n for n, _ in net.time_ops(1)]
    net.close()
    return names


def test_op_list_of_plain_224(tmp_path, hip_lib):
    names = op_names(tmp_path, "plain-224", "float16x3-wtower")
    assert names.count("tower_x3w") == 1 and names.count("block_x3w") == 1
    body = [n for n in names if n in ("tower_x3w", "block_x3w", "se_gate", "se")]
    assert body == ["tower_x3w", "se_gate", "block_x3w"], names
    old = op_names(tmp_path, "plain-224", "float16x3-wnet")
    assert "tower_x3w" not in old and old.count("block_x3w") == 3
    assert [n for n in names if n not in ("tower_x3w", "block_x3w")] == [n for n in old if n != "block_x3w"]


def test_op_list_of_a_gated_first_block(tmp_path, hip_lib):
    names = op_names(tmp_path, "run-224-gated-first", "float16x3-wtower")
    body = [n for n in names if n in ("tower_x3w", "block_x3w", "se_gate", "se")]
    assert body == ["block_x3w", "se_gate", "tower_x3w"], names
    old = op_names(tmp_path, "run-224-gated-first", "float16x3-wnet")
    assert "tower_x3w" not in old and old.count("block_x3w") == 4


def test_op_list_with_a_transformer_block_between_two_runs(tmp_path, hip_lib):
    names = op_names(tmp_path, "run-192-ntb", "float16x3-wtower")
    assert names.count("tower_x3w") == 2 and names.count("ntb_x3w") == 1 and "block_x3w" not in names
    body = [n for n in names if n in ("tower_x3w", "ntb_x3w")]
    assert body == ["tower_x3w", "ntb_x3w", "tower_x3w"], names
    old = op_names(tmp_path, "run-192-ntb", "float16x3-wnet")
    assert "tower_x3w" not in old and old.count("block_x3w") == 4 and old.count("ntb_x3w") == 1


def test_op_list_of_alphavile_normal(tmp_path, hip_lib):
    names = op_names(tmp_path, "alphavile-normal", "float16x3-wtower")
    assert names.count("tower_x3w") == 2 and names.count("ntb_x3w") == 2 and "block_x3w" not in names and "depthwise" not in names
    old = op_names(tmp_path, "alphavile-normal", "float16x3-wnet")
    assert "tower_x3w" not in old and old.count("ntb_x3w") == 2
    assert len(old) - len(names) == old.count("block_x3w") - 2


@pytest.mark.parametrize("batch", [1, 5, 256])
def test_batch_sizes(tmp_path, hip_lib, batch):
    x = nn_cases.synthetic_planes(batch, 52, 500 + batch)
    check(restatement("alphavile-tiny", x), *predict(tmp_path, "alphavile-tiny", "float16x3-wtower", x))


def test_two_runs_and_poisoned_lds_give_identical_bits(tmp_path, hip_lib, lds_poison):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    batch = 9
    x = nn_cases.synthetic_planes(batch, 52, 77).numpy().reshape(-1)
    net = HipAPI(0, batch, d, "float16x3-wtower")
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


@pytest.mark.parametrize("precision", ["float16x3-wtower", "float16p8-wtower"])
@pytest.mark.parametrize("kind", ["256-wide", "classical-192"])
def test_wtower_on_a_net_without_a_qualifying_block_is_refused(tmp_path, hip_lib, kind, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd = _unqualified(kind)
    d = nn_cases.export_case(tmp_path, kind, cfg, sd)
    with pytest.raises(Exception, match="`-wtower` runs the mobile-bottleneck and transformer blocks .* no block of this model qualifies"):
        HipAPI(0, 4, d, precision)
    if precision == "float16x3-wtower":
        HipAPI(0, 4, d, "float16x3").close()                       # (the same directory loads without the suffix)


@pytest.mark.parametrize("precision", ["float16x3-wtower", "float16p8-wtower"])
def test_an_expert_set_refuses_the_suffix(tmp_path, hip_lib, precision):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    assert not lib.mi_net_create_experts(root.encode(), 0, 8, precision.encode(), ec.LICHESS)
    assert "an expert set runs Precision float16x3" in _capi.last_error() and precision in _capi.last_error()
