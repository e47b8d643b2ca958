"""Precision float16x3's one-launch tower keeps the residual stream in the project waves' accumulators (exact f32; x3.hip:
x3_stream_load): a block adds its BN3 bias and its project sums onto it, SE gates squeeze it from the registers and scale it there.

What guards what:
  * roles vs symmetric, bit for bit: tower_x3_roles_kernel (EXPAND / PROJECT waves, the default) and tower_x3_kernel (every wave all three
    phases, CRA_X3_TOWER=symmetric) schedule the chunk pipeline differently and must still add every output in the same order.  Both call
    the same x3_stream_* helpers, so this test cannot see a bug INSIDE a helper (a wrong square or channel mapping in the load, squeeze, gate
    or store would be the same in both).
  * oracle parity at float32's 1e-4: what does see the helpers -- the stream's layout, the SE squeeze and gate of both kinds, the f32 result
    leaving from the registers -- on nets whose C_op is a multiple of 128 and on nets with a 64-channel remainder.
RISEv2-19 is the headline net (ca_se on its last five blocks); the five-block net puts eca_se and ca_se on consecutive blocks, a gated block
behind an ungated one and the run's last block gated."""
import numpy as np
import pytest
import torch

import nn_cases
from oracle import rise_oracle as ro

pytestmark = pytest.mark.gpu

TOL = dict(logit=1e-4, value=1e-4, prob=1e-6)


def _gated_runs():
    """Five 3x3 blocks, C_op 128 ... 384: gates of both kinds on consecutive blocks, a gated block right behind an ungated one and an
    ungated block behind a gated one; C_op % 128 = 64 on blocks 1 and 3."""
    cfg = ro.rise_v2_config(5, 34, 81)
    cfg.se_types = [None, "eca_se", "ca_se", None, "ca_se"]
    cfg.name = "risev2-5-gates"
    return cfg


def _net(tmp_path, name):
    if name == "risev2-5-gates":
        cfg = _gated_runs()
        sd = ro.make_state_dict(cfg, seed=31, stress=True)
        return cfg, sd, nn_cases.export_case(tmp_path, name, cfg, sd)
    cfg, sd, _ = nn_cases.make_case(name)
    return cfg, sd, nn_cases.export_case(tmp_path, name, cfg, sd)


def _predict(d, cfg, x, batch):
    from crazyara_amd.neuralnetapi import HipAPI
    net = HipAPI(0, batch, d, "float16x3-1wg", keep_logits=True)       # (-1wg: the one-launch tower at any batch)
    v, p = np.zeros(batch, np.float32), np.zeros(batch * cfg.nb_policy, np.float32)
    net.predict(x, v, p)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy()
    net.close()
    return v, p, logits


@pytest.mark.parametrize("name,batch", [("risev2-19", 12), ("risev2-5-gates", 7)])
def test_register_stream_two_role_tower_equals_the_symmetric_one_bit_for_bit(tmp_path, hip_lib, name, batch, monkeypatch):
    cfg, sd, d = _net(tmp_path, name)
    x = nn_cases.synthetic_planes(batch, cfg.nb_input_channels, 93).numpy().reshape(-1)
    outs = []
    for mode in ("roles", "symmetric"):
        monkeypatch.setenv("CRA_X3_TOWER", mode)
        outs.append(_predict(d, cfg, x, batch))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,batch", [("risev2-19", 6), ("risev2-5-gates", 5)])
def test_register_stream_tower_matches_the_oracle(tmp_path, hip_lib, name, batch):
    cfg, sd, d = _net(tmp_path, name)
    assert {c % 128 for c in cfg.channels_operating()} == {0, 64}
    x = nn_cases.synthetic_planes(batch, cfg.nb_input_channels, 94)
    value, probs, logits = _predict(d, cfg, np.ascontiguousarray(x.numpy()).reshape(-1), batch)
    o_value, o_logits, _ = ro.forward(cfg, sd, x)
    assert np.abs(value - o_value.numpy().reshape(-1)).max() < TOL["value"]
    assert np.abs(logits - o_logits.numpy()).max() < TOL["logit"]
    assert np.abs(probs.reshape(batch, -1) - torch.softmax(o_logits, dim=1).numpy()).max() < TOL["prob"]
