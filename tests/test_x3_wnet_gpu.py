"""GPU: precision "float16x3-wnet" -- "-wblock" plus every NextViT transformer block of a 128 / 192 / 224-channel net in one launch
(csrc/nn/x3_wntb.cpp: ntb_x3w_kernel<C>) instead of nine layer launches.

Held to the float16x3 bounds of tests/test_alphavile_gpu.py (TOL["float16x3"]: logits 1e-4, value 1e-4, probabilities 1e-6, aux 1e-4)
against the fp32 restatement and, for AlphaVile-tiny, the golden.  Against "float16x3-wblock" on the same net and inputs: the kernel walks
every sum in the layer kernels' order, so the outputs are the SAME BITS (array_equal; LAYER_PATH_BOUND = 2e-5 is the project's bound for
two float16x3 forms of one net, which bit equality meets with room).

The nets: ntb-128-eca (D = 96: 3 heads, M = 32: one group, H = 256: two whole chunks, an eca_se block right behind the NTB),
ntb-224-first-last (D = 160, M = 64: two groups, H = 448: the 64-channel tail chunk; an NTB reading the stem's output and an NTB the
heads read) and AlphaVile-tiny (C = 192) with its golden."""
import numpy as np
import pytest

import alphavile_oracle as ao
import nn_cases
from test_alphavile_gpu import REDUCED
from test_x3_wblock_gpu import LAYER_PATH_BOUND, cached_predict, case, check, predict, reference, restatement

pytestmark = pytest.mark.gpu

NETS = ("ntb-128-eca", "ntb-224-first-last", "alphavile-tiny")
FALLBACK = False          # ntb_x3w_kernel is one launch per NTB (not the two-kernel fallback)


@pytest.mark.parametrize("name", NETS)
def test_predict_matches_the_restatement_and_the_golden(tmp_path, hip_lib, name):
    check(reference(name), *cached_predict(tmp_path, name, "float16x3-wnet"), golden=case(name)[5])


@pytest.mark.parametrize("name", NETS)
def test_wnet_gives_the_bits_of_wblock(tmp_path, hip_lib, name):
    """the same products in the same f32 summation order as the nine layer launches"""
    layer = cached_predict(tmp_path, name, "float16x3-wblock")
    fused = cached_predict(tmp_path, name, "float16x3-wnet")
    d = float(np.abs(layer[3] - fused[3]).max())
    dv = float(np.abs(layer[0] - fused[0]).max())
    print(f"{name}: max |logits(float16x3-wnet) - logits(float16x3-wblock)| = {d:.3e}; value {dv:.3e}")
    assert d < LAYER_PATH_BOUND and dv < LAYER_PATH_BOUND
    assert np.array_equal(layer[3], fused[3]) and np.array_equal(layer[0], fused[0])


@pytest.mark.parametrize("batch", [1, 5, 256])
def test_batch_sizes(tmp_path, hip_lib, batch):
    x = nn_cases.synthetic_planes(batch, 52, 500 + batch)
    check(restatement("alphavile-tiny", x), *predict(tmp_path, "alphavile-tiny", "float16x3-wnet", x))


@pytest.mark.parametrize("name", ["ntb-224-first-last", "alphavile-normal"])
def test_op_list_has_one_launch_per_block_and_per_ntb(tmp_path, hip_lib, name):
    from crazyara_amd.neuralnetapi import HipAPI
    if name in REDUCED:
        cfg, sd, _, _, _, _ = case(name)
    else:
        cfg, sd, _ = ao.make_case(name)
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version="3.0")
    lists = {}
    for prec in ("float16x3-wnet", "float16x3-wblock"):
        net = HipAPI(0, 4, d, prec)
        lists[prec] = [n for n, _ in net.time_ops(1)]
        net.close()
    names, old = lists["float16x3-wnet"], lists["float16x3-wblock"]
    ntbs = sum(bool(cfg.transformer(i)) for i in range(len(cfg.kernels)))
    assert ntbs >= 2
    assert names.count("ntb_x3w") == (2 if FALLBACK else 1) * ntbs
    assert "attention" not in names
    assert names.count("block_x3w") == len(cfg.kernels) - ntbs
    assert len(old) - len(names) == (7 if FALLBACK else 8) * ntbs
    assert old.count("attention") == ntbs and "ntb_x3w" not in old            # the old suffix is untouched


def test_two_runs_and_poisoned_lds_give_identical_bits(tmp_path, hip_lib, lds_poison):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    batch = 9
    x = nn_cases.synthetic_planes(batch, 52, 77).numpy().reshape(-1)
    net = HipAPI(0, batch, d, "float16x3-wnet")
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


def test_float16p8_wnet_gives_the_bits_of_float16x3_wnet(tmp_path, hip_lib):
    a = cached_predict(tmp_path, "alphavile-tiny", "float16x3-wnet")
    b = predict(tmp_path, "alphavile-tiny", "float16p8-wnet")
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


@pytest.mark.parametrize("precision", ["float32-wnet", "float16-wnet", "fp8-wnet", "int8-wnet"])
def test_wnet_on_another_precision_is_refused(tmp_path, hip_lib, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    with pytest.raises(Exception, match="`-wnet` is a float16x3 kernel family"):
        HipAPI(0, 4, d, precision)


@pytest.mark.parametrize("kind", ["256-wide", "classical-192"])
def test_wnet_on_a_net_without_a_qualifying_block_is_refused(tmp_path, hip_lib, kind):
    from crazyara_amd.neuralnetapi import HipAPI
    from test_x3_wblock_gpu import _unqualified
    cfg, sd = _unqualified(kind)
    d = nn_cases.export_case(tmp_path, kind, cfg, sd)
    with pytest.raises(Exception, match="no block of this model qualifies"):
        HipAPI(0, 4, d, "float16x3-wnet")


@pytest.mark.parametrize("precision", ["float16x3-wnet", "float16p8-wnet"])
def test_an_expert_set_refuses_the_suffix(tmp_path, hip_lib, precision):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    assert not lib.mi_net_create_experts(root.encode(), 0, 8, precision.encode(), ec.LICHESS)
    assert "an expert set runs Precision float16x3" in _capi.last_error() and precision in _capi.last_error()


def test_a_net_without_an_ntb_builds_the_op_list_of_wblock(tmp_path, hip_lib):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("plain-224")
    d = nn_cases.export_case(tmp_path, "plain-224", cfg, sd, version=version)
    lists = []
    for prec in ("float16x3-wnet", "float16x3-wblock"):
        net = HipAPI(0, 4, d, prec)
        lists.append([n for n, _ in net.time_ops(1)])
        net.close()
    assert lists[0] == lists[1] and "block_x3w" in lists[0]
