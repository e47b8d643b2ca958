"""GPU: precision "float16x3-wsplit" -- "-wnet", and in a net made for at most 64 boards every mobile-bottleneck block of a 128 / 192 /
224-channel net over G workgroups per board (csrc/nn/x3_wsplit.cpp: block_x3w_split_kernel<C, KS>, x3w_split_finish_kernel).

Held to the float16x3 bounds of tests/test_alphavile_gpu.py (TOL["float16x3"]: logits 1e-4, value 1e-4, probabilities 1e-6, aux 1e-4)
against the fp32 restatement and, for AlphaVile-tiny, the golden.  Against "float16x3-wnet" on the same net and inputs the logits and the
value stay within LAYER_PATH_BOUND = 2e-5, the project's bound for two float16x3 forms of one net: G shares compute the same products and
add the project sums of their chunks in another order.  ONE share is block_x3w_kernel's arithmetic: the nets whose blocks are a single
chunk give float16x3-wnet's bits.

The nets: plain-224 (C_op 448: three chunks and the 64-channel tail, G = 4; a 5x5 block, an image-to-image hand-over, a gated last block
in front of the heads), ntb-224-first-last (a block between two transformer blocks), ntb-128-eca (two chunks, a gated block behind a
transformer block), AlphaVile-tiny with its golden, mobile-128 / mobile-192 (C_op 64 / 96 / 128: G = 1; ca_se, eca_se, 5x5) and
wide-op-128 (C_op 640: five chunks, so that 4 shares are uneven -- 1, 1, 1, 2 chunks -- at batch 64 and G = 5 at batch 8)."""
import numpy as np
import pytest

import alphavile_oracle as ao
import nn_cases
from crazyara_amd import rise_config as rc
from test_x3_wblock_gpu import LAYER_PATH_BOUND, cached_predict, case, check, mobile, predict, reference, restatement

pytestmark = pytest.mark.gpu

NETS = ("plain-224", "ntb-224-first-last", "ntb-128-eca", "alphavile-tiny")
SPLIT_OPS = {"block_x3w_split", "x3w_split_finish"}


@pytest.mark.parametrize("name", NETS)
def test_predict_matches_the_restatement_and_the_golden(tmp_path, hip_lib, name):
    check(reference(name), *cached_predict(tmp_path, name, "float16x3-wsplit"), golden=case(name)[5])


@pytest.mark.parametrize("name", NETS)
def test_logits_and_value_stay_within_the_bound_of_two_float16x3_forms(tmp_path, hip_lib, name):
    """float16x3-wnet (one workgroup per board) and float16x3-wsplit: the same products, the chunks' project sums added share by share"""
    one = cached_predict(tmp_path, name, "float16x3-wnet")
    split = cached_predict(tmp_path, name, "float16x3-wsplit")
    d = float(np.abs(one[3] - split[3]).max())
    dv = float(np.abs(one[0] - split[0]).max())
    print(f"{name}: max |logits(float16x3-wsplit) - logits(float16x3-wnet)| = {d:.3e}; value {dv:.3e}")
    assert d < LAYER_PATH_BOUND and dv < LAYER_PATH_BOUND


@pytest.mark.parametrize("name", ["mobile-128", "mobile-192"])
def test_a_single_share_gives_the_bits_of_wnet(tmp_path, hip_lib, name):
    """every block of these nets is one chunk, G = 1: block_x3w_kernel's sums in its order, its gates from its channel sums"""
    assert mobile(128).se_types[1:] == ["ca_se", "eca_se"] and mobile(128).kernels == [3, 5, 3]
    one = cached_predict(tmp_path, name, "float16x3-wnet")
    split = cached_predict(tmp_path, name, "float16x3-wsplit")
    print(f"{name}: max |logits(float16x3-wsplit) - logits(float16x3-wnet)| = {float(np.abs(one[3] - split[3]).max()):.3e}")
    assert np.array_equal(one[0], split[0]) and np.array_equal(one[1], split[1]) and np.array_equal(one[3], split[3])
    check(reference(name), *split)


def wide_op():
    """two 3x3 blocks of C_op 640 on 128 channels: five chunks (tests/test_alphavile_gpu.py's reduced() otherwise)"""
    return rc.RiseConfig(nb_input_channels=52, channels=128, channels_operating_init=640, channel_expansion=0, kernels=[3, 3],
                         se_types=[None, None], value_fc_size=128, channels_policy_head=76, use_transformers=[False, False],
                         name="wide-op-128")


@pytest.mark.parametrize("batch", [64, 8])
def test_uneven_shares_match_the_restatement(tmp_path, hip_lib, batch):
    """batch 64: G = 4, shares of 1, 1, 1 and 2 chunks; batch 8: G = 5"""
    from test_x3_wblock_gpu import _cases
    if "wide-op-128" not in _cases:
        cfg = wide_op()
        assert cfg.channels_operating_init // 128 == 5
        sd = rc.make_state_dict(cfg, seed=44)
        sd["policy_head.body.3.weight"] = sd["policy_head.body.3.weight"] * 0.5       # (as the plain net of REDUCED: seeded logits of +-6 otherwise)
        _cases["wide-op-128"] = (cfg, sd, nn_cases.synthetic_planes(5, 52, 44), "3.0", ao.forward, None)
    x = nn_cases.synthetic_planes(batch, 52, 600 + batch)
    check(restatement("wide-op-128", x), *predict(tmp_path, "wide-op-128", "float16x3-wsplit", x))


def test_the_same_share_count_gives_the_same_bits_whatever_the_batch(tmp_path, hip_lib):
    """plain-224 has G = 4 at 3 and at 4 boards: a board's result does not depend on the boards beside it"""
    x = case("plain-224")[2]
    four = predict(tmp_path, "plain-224", "float16x3-wsplit", x[:4])
    three = predict(tmp_path, "plain-224", "float16x3-wsplit", x[:3])
    for k in (0, 1, 3):
        assert np.array_equal(four[k][:3], three[k])


def test_two_runs_and_poisoned_lds_give_identical_bits(tmp_path, hip_lib, lds_poison):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    batch = 9
    x = nn_cases.synthetic_planes(batch, 52, 77).numpy().reshape(-1)
    net = HipAPI(0, batch, d, "float16x3-wsplit")
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


def test_float16p8_wsplit_gives_the_bits_of_float16x3_wsplit(tmp_path, hip_lib):
    a = cached_predict(tmp_path, "alphavile-tiny", "float16x3-wsplit")
    b = predict(tmp_path, "alphavile-tiny", "float16p8-wsplit")
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


def op_names(tmp_path, name, precision, batch):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case(name)
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version=version)
    net = HipAPI(0, batch, d, precision)
    names = [n for n, _ in net.time_ops(1)]
    net.close()
    return names


def expected_body(cfg):
    """the launches between the stem and the heads: a finish launch exactly in front of whatever reads the float stream"""
    body, images = [], False
    for i in range(len(cfg.kernels)):
        if cfg.transformer(i):
            body += (["x3w_split_finish"] if images else []) + ["ntb_x3w"]
            images = False
            continue
        if cfg.se_types[i]:                                # a gated block: its gate from the stream's channel sums, or the in-place SE launch
            body += ["x3w_split_finish", "se_gate"] if images else ["se"]
        body.append("block_x3w_split")
        images = True
    return body + (["x3w_split_finish"] if images else [])


@pytest.mark.parametrize("name", NETS)
def test_op_list_has_a_split_launch_per_block_and_a_finish_in_front_of_every_reader_of_the_stream(tmp_path, hip_lib, name):
    cfg = case(name)[0]
    names = op_names(tmp_path, name, "float16x3-wsplit", 4)
    old = op_names(tmp_path, name, "float16x3-wnet", 4)
    ntbs = sum(bool(cfg.transformer(i)) for i in range(len(cfg.kernels)))
    gated = sum(bool(cfg.se_types[i]) and not cfg.transformer(i) for i in range(len(cfg.kernels)))
    assert names.count("block_x3w_split") == len(cfg.kernels) - ntbs == old.count("block_x3w")
    assert "block_x3w" not in names and names.count("ntb_x3w") == ntbs == old.count("ntb_x3w")
    body = expected_body(cfg)
    first = min(i for i, n in enumerate(names) if n in SPLIT_OPS | {"ntb_x3w", "se"})
    assert names[first:first + len(body)] == body, (names, body)
    assert names[:first] == old[:first]                                        # the stem
    heads = names[first + len(body):]
    assert heads and not SPLIT_OPS & set(heads) and heads == old[len(old) - len(heads):]      # the heads: -wnet's launches
    assert names.count("se") + names.count("se_gate") == gated == old.count("se") + old.count("se_gate")
    assert not SPLIT_OPS & set(old)                                           # the old suffix is untouched


def test_a_net_made_for_more_than_64_boards_builds_the_op_list_of_wnet(tmp_path, hip_lib):
    names = op_names(tmp_path, "ntb-128-eca", "float16x3-wsplit", 65)
    assert names == op_names(tmp_path, "ntb-128-eca", "float16x3-wnet", 65) and "block_x3w" in names and not SPLIT_OPS & set(names)
    assert "block_x3w_split" in op_names(tmp_path, "ntb-128-eca", "float16x3-wsplit", 64)


def test_few_boards_on_a_net_made_for_many_take_the_split_board_forward(tmp_path, hip_lib):
    """a float16x3-wsplit net made for 128 boards hands a call of 8 boards to its companion net, which is made from the same precision
    string: the bits of a float16x3-wsplit net made for 8 boards (G follows the boards of the call)"""
    import ctypes as C
    from crazyara_amd import _capi, env, openings
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _, version, _, _ = case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version=version)
    lib = _capi.load()
    n = 8
    layout = env.planes_layout(1, "3.0")
    fens = openings.position_fens("chess")
    pos = [env.Position(f, False, "chess") for f in fens[::len(fens) // n][:n]]
    assert len(pos) == n
    descs = b"".join(p.desc(layout) for p in pos)
    outs = {}
    for batch in (128, n):
        net = HipAPI(0, batch, d, "float16x3-wsplit")
        v = np.full(batch, 7.0, np.float32)
        p = np.full(batch * cfg.nb_policy, 7.0, np.float32)
        assert lib.mi_net_submit_boards(net._h, descs, n, layout, v.ctypes.data, p.ctypes.data, None) == 0, _capi.last_error()
        net.wait()
        outs[batch] = (v[:n].copy(), p[:n * cfg.nb_policy].copy())
        net.close()
    assert np.isfinite(outs[n][0]).all() and np.abs(outs[n][0]).max() <= 1.0 and abs(outs[n][1].reshape(n, -1).sum(1) - 1.0).max() < 1e-4
    assert np.array_equal(outs[128][0], outs[n][0]) and np.array_equal(outs[128][1], outs[n][1])
    planes = np.stack([q.planes(1, "3.0", True) for q in pos]).astype(np.float32)
    import torch
    ref = restatement("alphavile-tiny", torch.from_numpy(planes))
    assert np.abs(outs[n][0] - ref[0]).max() < 1e-4


@pytest.mark.parametrize("precision", ["float16x3-wsplit", "float16p8-wsplit"])
@pytest.mark.parametrize("kind", ["256-wide", "classical-192"])
def test_wsplit_on_a_net_without_a_qualifying_block_is_refused(tmp_path, hip_lib, kind, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    from test_x3_wblock_gpu import _unqualified
    cfg, sd = _unqualified(kind)
    d = nn_cases.export_case(tmp_path, kind, cfg, sd)
    with pytest.raises(Exception, match="`-wnet` runs the mobile-bottleneck and transformer blocks .* no block of this model qualifies"):
        HipAPI(0, 4, d, precision)


@pytest.mark.parametrize("precision", ["float16x3-wsplit", "float16p8-wsplit"])
def test_an_expert_set_refuses_the_suffix(tmp_path, hip_lib, precision):
    import experts_cases as ec
    from crazyara_amd import _capi
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    assert not lib.mi_net_create_experts(root.encode(), 0, 8, precision.encode(), ec.LICHESS)
    assert "an expert set runs Precision float16x3" in _capi.last_error() and precision in _capi.last_error()
