"""Precision float16x3, nets made for more than 64 boards: the policy chain with the value head on the two waves that have no cout tile in
its second conv (x3_heads.cpp: conv3x3_x3_heads_kernel, the default) against the two launches it replaces (x3.hip: conv3x3_x3_chain_kernel
+ kernels.hip: value_head_kernel_8w, CRA_X3_HEADS_APART=1) and against the float64-folded oracle.

The new kernel is the chain step for step and the value head's arithmetic term for term on other threads, so value, probabilities and
logits are asked to be IDENTICAL arrays, and both forms inside float16x3's bounds of tests/test_nn_parity_gpu.py.  That the two runs are
two kernels is asserted through HipAPI.time_ops / op_kernels, not assumed.

Cases, the smallest that reach every edge: 65 boards (the first batch above the threshold) on a 3-block net whose blocks are all gated,
72 boards on RISEv2-7, the lichess tables (80 input planes; 84 policy channels = six cout tiles with 12 padded couts); logits kept and
not kept; a forward of 65 boards on a net made for 72 (an expert set's group); the nets the fused form must leave alone; run to run."""
import numpy as np
import pytest
import torch

import experts_cases as ec
import nn_cases
from oracle import rise_oracle as ro
from test_nn_parity_gpu import TOL

pytestmark = pytest.mark.gpu

HEADS, CHAIN = "conv3x3_x3_heads_kernel", "conv3x3_x3_chain_kernel"
SWITCHES = ("CRA_X3_HEADS_APART", "CRA_X3_VALUE_HEAD", "CRA_VALUE_HEAD_VARIANT", "CRA_X3_NO_HEAD_CHAIN")


def _all_gated():
    cfg = ro.rise_v2_config(3, 34, 81)
    cfg.se_types = ["ca_se", "eca_se", "ca_se"]
    cfg.name = "risev2-3-all-gated"
    return cfg


def _wide_policy():
    cfg = ro.rise_v2_config(3, 34, 100)            # 100 policy channels: 112 padded couts, seven cout tiles -- the second conv uses wave 6
    cfg.name = "risev2-3-p100"
    return cfg


OWN = {"risev2-3-all-gated": (_all_gated, 51), "risev2-3-p100": (_wide_policy, 52)}


def _case(tmp_path, name):
    if name in OWN:
        cfg = OWN[name][0]()
        sd = ro.make_state_dict(cfg, seed=OWN[name][1], stress=True)
    else:
        cfg, sd, _ = nn_cases.make_case(name)
    return cfg, sd, nn_cases.export_case(tmp_path, name, cfg, sd, version="3.0" if cfg.nb_input_channels in (52, 64, 80) else "1.0")


def _env(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _structure(net):
    return [n for n, _ in net.time_ops(1)], net.op_kernels()


def _forward(d, cfg, xin, batch, keep_logits=True, calls=2, precision="float16x3"):
    from crazyara_amd.neuralnetapi import HipAPI
    net = HipAPI(0, batch, d, precision, keep_logits=keep_logits)
    names, kernels = _structure(net)
    outs = []
    for _ in range(calls):
        v, p = np.full(batch, 7.0, np.float32), np.full(batch * cfg.nb_policy, 7.0, np.float32)
        net.predict(xin, v, p, np.full(batch * 4, 7.0, np.float32) if cfg.nb_aux else None)
        logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy().copy() if keep_logits else None
        outs.append((v, p, logits))
    net.close()
    return names, kernels, outs


def _assert_fused(names, kernels):
    assert names[-1] == "conv_gemm_x3_3x3" and "value_head" not in names, names
    assert kernels[-1] == HEADS and CHAIN not in kernels, kernels


def _assert_apart(names, kernels):
    assert names[-2:] == ["conv_gemm_x3_3x3", "value_head"], names
    assert kernels[-2:] == [CHAIN, "value_head"] and HEADS not in kernels, kernels


@pytest.mark.parametrize("name,batch,seed", [("risev2-3-all-gated", 65, 201), ("risev2-7", 72, 202), ("risev2-13-lichess", 65, 203)])
def test_same_bits_as_the_two_launches_and_two_different_kernels(tmp_path, hip_lib, monkeypatch, name, batch, seed):
    cfg, sd, d = _case(tmp_path, name)
    x = nn_cases.synthetic_planes(batch, cfg.nb_input_channels, seed)         # (every board differs)
    xin = np.ascontiguousarray(x.numpy())
    _env(monkeypatch)
    names, kernels, new = _forward(d, cfg, xin, batch)
    _assert_fused(names, kernels)
    _env(monkeypatch, CRA_X3_HEADS_APART="1")
    names_old, kernels_old, old = _forward(d, cfg, xin, batch)
    _assert_apart(names_old, kernels_old)
    assert names[:-1] == names_old[:-2] and kernels[:-1] == kernels_old[:-2]
    for (v, p, lg), (v0, p0, lg0) in zip(new, old):
        assert np.array_equal(v, v0), np.abs(v - v0).max()
        assert np.array_equal(p, p0)
        assert np.array_equal(lg, lg0)
    assert np.array_equal(new[0][0], new[1][0]) and np.array_equal(new[0][1], new[1][1])
    o_value, o_logits, _ = ro.forward(cfg, sd, x)
    tol = TOL["float16x3"]
    for what, (v, p, lg) in (("heads", new[1]), ("apart", old[1])):
        e_v = float(np.abs(v - o_value.numpy().reshape(-1)).max())
        e_l = float(np.abs(lg.reshape(batch, -1) - o_logits.numpy()).max())
        e_p = float(np.abs(p.reshape(batch, -1) - torch.softmax(o_logits, 1).numpy()).max())
        print(name, batch, what, "value", e_v, "logits", e_l, "probs", e_p)
        assert e_v < tol["value"] and e_l < tol["logit"] and e_p < tol["prob"], what
    assert len({float(t) for t in new[1][0]}) > batch // 2                   # the values differ from board to board: a swapped slot would show


def test_logits_kept_and_not_kept(tmp_path, hip_lib, monkeypatch):
    cfg, sd, d = _case(tmp_path, "risev2-3")
    xin = np.ascontiguousarray(nn_cases.synthetic_planes(65, cfg.nb_input_channels, 204).numpy())
    _env(monkeypatch)
    _, kernels, kept = _forward(d, cfg, xin, 65, keep_logits=True)
    _, kernels_not, dropped = _forward(d, cfg, xin, 65, keep_logits=False)
    assert kernels[-1] == HEADS and kernels_not[-1] == HEADS
    assert np.array_equal(kept[1][0], dropped[1][0]) and np.array_equal(kept[1][1], dropped[1][1])
    assert np.isfinite(kept[1][0]).all() and np.isfinite(kept[1][1]).all()


def test_a_forward_of_fewer_boards_than_the_net_was_made_for(tmp_path, hip_lib, monkeypatch):
    """An expert set's group of 65 boards on experts made for 72: the group runs the full-size net's launches with the boards of the call
    (ForwardCall::boards), the new kernel on 65 workgroups.  65 is the smallest such forward there is: an expert set runs plain float16x3
    only, and there a group of at most 64 boards goes to the companion net made for 64, which keeps its own heads.  The caller's value and
    probability entries behind board 65 keep what they held."""
    from crazyara_amd.neuralnetapi import HipAPI, HipExperts
    n = 65
    root, dirs = ec.export_experts(tmp_path, case="risev2-3")
    pools = ec.positions_by_phase((n, 0, 0))
    positions = ec.make_batch(pools, (n, 0, 0), seed=3)
    got = {}
    for apart in (False, True):
        _env(monkeypatch, **({"CRA_X3_HEADS_APART": "1"} if apart else {}))
        plain = HipAPI(0, 72, dirs[0], "float16x3")
        names, kernels = _structure(plain)
        plain.close()
        (_assert_apart if apart else _assert_fused)(names, kernels)
        experts = HipExperts(0, 72, root, "float16x3", ec.LICHESS)
        buf = ec.CallBuffers.for_net(experts, "risev2-3")
        buf.load(positions)
        assert list(experts.route_phases(buf.p_desc, n)) == [0] * n
        buf.poison()
        buf.submit_boards(experts, n)
        got[apart] = (buf.value.copy(), buf.probs.copy())
        buf.close()
        experts.close()
    npol = len(got[False][1]) // 72
    for value, probs in got.values():
        assert np.isfinite(value[:n]).all() and np.isfinite(probs[:n * npol]).all()
        assert np.all(value[n:].view(np.uint32) == ec.POISON) and np.all(probs[n * npol:].view(np.uint32) == ec.POISON)
    assert np.array_equal(got[False][0][:n], got[True][0][:n])
    assert np.array_equal(got[False][1][:n * npol], got[True][1][:n * npol])
    assert len({float(t) for t in got[False][0][:n]}) > n // 2


@pytest.mark.parametrize("name,batch,env", [
    ("risev33-wdlp", 65, {}),                                   # the WDLP value head
    ("risev2-3", 64, {}),                                       # at most 64 boards: heads_small / value_head stay
    ("risev2-3", 65, {"CRA_X3_VALUE_HEAD": "one"}),             # a value head kernel asked for by name
    ("risev2-3-p100", 65, {}),                                  # seven cout tiles: the second conv uses wave 6
])
def test_nets_the_fused_form_leaves_alone(tmp_path, hip_lib, monkeypatch, name, batch, env):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, d = _case(tmp_path, name)
    _env(monkeypatch, **env)
    net = HipAPI(0, batch, d, "float16x3-1wg")                  # (-1wg: the 64-board net keeps value_head instead of heads_small)
    names, kernels = _structure(net)
    net.close()
    assert "value_head" in names and HEADS not in kernels, (names, kernels)


def test_run_to_run_and_net_to_net(tmp_path, hip_lib, monkeypatch):
    cfg, sd, d = _case(tmp_path, "risev2-3")
    xin = np.ascontiguousarray(nn_cases.synthetic_planes(65, cfg.nb_input_channels, 205).numpy())
    _env(monkeypatch)
    runs = []
    for _ in range(2):
        _, kernels, outs = _forward(d, cfg, xin, 65, calls=3)
        assert kernels[-1] == HEADS
        runs += outs
    for v, p, lg in runs[1:]:
        assert np.array_equal(v, runs[0][0]) and np.array_equal(p, runs[0][1]) and np.array_equal(lg, runs[0][2])
