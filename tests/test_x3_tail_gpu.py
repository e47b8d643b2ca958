"""Precision float16x3's two-role tower runs the last chunk of a block at 64 channels when C_op % 128 == 64 (x3_tail.cpp:
tower_x3_tail_kernel, the default) instead of paying a whole 128-channel chunk whose upper half is zero padding
(x3.hip: tower_x3_roles_kernel, CRA_X3_NO_TAIL=1).

The padded channels contribute exact zeros and the real channels are summed in the order they were, so the two kernels must agree BIT FOR
BIT on value, probabilities, logits and the auxiliary outputs; the old kernel is the reference.  Both kernels share their device helpers
(x3_device.h), so each case also holds the logits to the float64-folded oracle at float16x3's bounds (tests/test_nn_parity_gpu.py: TOL).

The cases: both parities of C_op at a small batch and at more boards than one wave of workgroups' worth of a small GPU partition; gates of
both kinds in front of and behind a tail block; a block that is ONLY a tail (C_op = 64: the first expand interval is the tail's); the 5x5
depthwise with a half chunk (RISEv3.3: C_op 416 and 448 on its 5x5 blocks, 288 / 320 / 544 on 3x3 ones); the headline net at its
benchmark batch."""
import numpy as np
import pytest
import torch

import nn_cases
from oracle import rise_oracle as ro

pytestmark = pytest.mark.gpu

TOL = dict(logit=1e-4, value=1e-4, prob=1e-6, aux=1e-4)          # tests/test_nn_parity_gpu.py: TOL["float16x3"] = TOL["float32"]


def _gates():
    """Five 3x3 blocks, C_op 128, 192, 256, 320, 384 (tests/test_x3_stream_gpu.py): tails on blocks 1 and 3; block 2 (ca_se) follows the
    tail block 1, which is itself gated (eca_se); the tail block 3 follows the gated block 2 and the gated block 4 follows it."""
    cfg = ro.rise_v2_config(5, 34, 81)
    cfg.se_types = [None, "eca_se", "ca_se", None, "ca_se"]
    cfg.name = "risev2-5-gates"
    return cfg, 31


def _tail_only_first():
    """Three 3x3 blocks, C_op 64, 128, 192: the first block is one 64-channel chunk, the last a tail behind a gate."""
    cfg = ro.rise_v2_config(3, 34, 81)
    cfg.channels_operating_init = 64
    cfg.se_types = [None, None, "ca_se"]
    cfg.name = "risev2-3-cop64"
    return cfg, 37


OWN = {"risev2-5-gates": _gates, "risev2-3-cop64": _tail_only_first}


def _net(tmp_path, name):
    if name in OWN:
        cfg, seed = OWN[name]()
        sd = ro.make_state_dict(cfg, seed=seed, stress=True)
    else:
        cfg, sd, _ = nn_cases.make_case(name)
    return cfg, sd, nn_cases.export_case(tmp_path, name, cfg, sd, version="3.0" if cfg.nb_input_channels in (52, 64, 80) else "1.0")


def _predict(d, cfg, x, batch, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    net = HipAPI(0, batch, d, precision, keep_logits=True)
    names = [n for n, _ in net.time_ops(1)]
    v, p = np.full(batch, 7.0, np.float32), np.full(batch * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(batch * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(x, v, p, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy().copy()
    net.close()
    return names, (v, p, logits, aux)


@pytest.mark.parametrize("name,batch,precision,oracle", [
    ("risev2-7", 3, "float16x3-1wg", True),           # C_op 128 ... 512, both parities, the tower kernel at a small batch
    ("risev2-7", 72, "float16x3", True),
    ("risev2-5-gates", 7, "float16x3-1wg", True),
    ("risev2-3-cop64", 5, "float16x3-1wg", True),
    ("risev33-wdlp", 8, "float16x3-1wg", True),       # 5x5 runs with a half chunk; WDLP head: the auxiliary outputs
    ("risev2-19", 256, "float16x3", False),           # the headline: bit-equal only
])
def test_tail_chunk_tower_equals_the_full_chunk_tower_bit_for_bit(tmp_path, hip_lib, name, batch, precision, oracle, monkeypatch):
    cfg, sd, d = _net(tmp_path, name)
    assert any(-c % 128 >= 64 for c in cfg.channels_operating())       # a block whose padding is half a chunk or more
    x = nn_cases.synthetic_planes(batch, cfg.nb_input_channels, 95)
    xin = np.ascontiguousarray(x.numpy()).reshape(-1)
    monkeypatch.delenv("CRA_X3_NO_TAIL", raising=False)
    names, new = _predict(d, cfg, xin, batch, precision)
    monkeypatch.setenv("CRA_X3_NO_TAIL", "1")
    names_old, old = _predict(d, cfg, xin, batch, precision)
    assert names == names_old and "tower_x3" in names, (names, names_old)
    for a, b in zip(new, old):
        assert (a is None and b is None) or np.array_equal(a, b)
    if oracle:
        value, probs, logits, aux = new
        o_value, o_logits, o_aux = ro.forward(cfg, sd, x)
        print(name, batch, "logit", np.abs(logits - o_logits.numpy()).max(), "value", np.abs(value - o_value.numpy().reshape(-1)).max())
        assert np.abs(logits - o_logits.numpy()).max() < TOL["logit"]
        assert np.abs(value - o_value.numpy().reshape(-1)).max() < TOL["value"]
        assert np.abs(probs.reshape(batch, -1) - torch.softmax(o_logits, dim=1).numpy()).max() < TOL["prob"]
        if cfg.nb_aux:
            assert np.abs(aux.reshape(-1, 4) - o_aux.numpy()).max() < TOL["aux"]
