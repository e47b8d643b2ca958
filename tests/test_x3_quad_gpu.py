"""Precision float16x3's two-role tower with transposed expand accumulators (x3_quad.cpp: tower_x3_quad_kernel, the default of 3x3 runs)
against the kernel it is a sibling of (x3_tail.cpp: tower_x3_tail_kernel, CRA_X3_NO_QUAD=1) and against the float64-folded oracle, on
value, probabilities, logits and the WDLP outputs.

The two kernels add the same products in the same order, but the expand MFMAs take their operands swapped and the accumulation inside an
MFMA is not specified to be the same then, so bit equality is not demanded.  The bounds:
  1. both kernels hold every output to the oracle at float16x3's bounds (tests/test_nn_parity_gpu.py: TOL["float16x3"]);
  2. the new kernel's largest logit difference from the tail kernel is no larger than the tail kernel's own largest deviation from the
     oracle on the same net and boards (both printed).
That the two runs are two kernels is asserted, not assumed: HipAPI.op_kernels() names the kernel every launch goes to.

The cases are the smallest at which the kernel can go wrong: 1 and 3 boards on RISEv2 nets of 2 and 3 blocks (C_op 128: one full chunk,
192: a full chunk and a tail, 256: two chunks); a net whose first block is gated and one gated in mid-run (the gate phases on the
unchanged square order); the WDLP head (its 5x5 runs stay on the tail kernel, its 3x3 runs are the new kernel's); 64 boards that differ
from a common base in ONE square each, every square once -- a misrouted halo value or a wrong row shows at a named square; 19 blocks at
8 boards."""
import numpy as np
import pytest
import torch

import nn_cases
from oracle import rise_oracle as ro

pytestmark = pytest.mark.gpu

TOL = dict(logit=1e-4, value=1e-4, prob=1e-6, aux=1e-4)          # tests/test_nn_parity_gpu.py: TOL["float16x3"] = TOL["float32"]


def _v2(nblocks, se_types, seed, name):
    def make():
        cfg = ro.rise_v2_config(nblocks, 34, 81)
        cfg.se_types = list(se_types)
        cfg.name = name
        return cfg, seed
    return make


OWN = {
    "risev2-2": _v2(2, [None, None], 41, "risev2-2"),                               # C_op 128, 192
    "risev2-3-plain": _v2(3, [None, None, None], 42, "risev2-3-plain"),             # C_op 128, 192, 256
    "risev2-3-gate-first": _v2(3, ["ca_se", None, None], 43, "risev2-3-gate-first"),
    "risev2-3-gate-mid": _v2(3, [None, "eca_se", "ca_se"], 44, "risev2-3-gate-mid"),
}


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
    kernels = net.op_kernels()                                     # the kernel every launch goes to (mi_net_op_kernel)
    v, p = np.full(batch, 7.0, np.float32), np.full(batch * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(batch * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(x, v, p, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy().copy()
    net.close()
    return names, kernels, (v, p, logits, aux)


def _one_square_boards(channels, seed):
    """64 boards: a common base, board i with one more piece-like entry on square i of a plane that is empty there."""
    base = nn_cases.synthetic_planes(1, channels, seed)
    x = base.repeat(64, 1, 1, 1).clone()
    for sq in range(64):
        r, f = divmod(sq, 8)
        plane = next(c for c in range(channels) if float(base[0, c, r, f]) == 0.0)
        x[sq, plane, r, f] = 1.0
    return x


QUAD, TAIL = "tower_x3_quad_kernel<3>", "tower_x3_tail_kernel<3>"


def _check(tmp_path, monkeypatch, name, batch, x=None, peaked=False):
    cfg, sd, d = _net(tmp_path, name)
    if x is None:
        x = nn_cases.synthetic_planes(batch, cfg.nb_input_channels, 97)
    xin = np.ascontiguousarray(x.numpy()).reshape(-1)
    monkeypatch.delenv("CRA_X3_NO_QUAD", raising=False)
    monkeypatch.delenv("CRA_X3_NO_TAIL", raising=False)
    names, kernels, new = _predict(d, cfg, xin, batch, "float16x3-1wg")
    monkeypatch.setenv("CRA_X3_NO_QUAD", "1")
    names_old, kernels_old, old = _predict(d, cfg, xin, batch, "float16x3-1wg")
    assert names == names_old and "tower_x3" in names, (names, names_old)
    # the comparison below is between two kernels only if the default's 3x3 runs went to the new one and the switch's to its sibling:
    # every launch the same but for those (5x5 runs, the WDLP net's, are tower_x3_tail_kernel<5> in both)
    assert QUAD in kernels and TAIL not in kernels, kernels
    assert TAIL in kernels_old and QUAD not in kernels_old, kernels_old
    assert [TAIL if k == QUAD else k for k in kernels] == kernels_old, (kernels, kernels_old)
    o_value, o_logits, o_aux = ro.forward(cfg, sd, x)
    o_logits, o_value = o_logits.numpy(), o_value.numpy().reshape(-1)
    o_probs = torch.softmax(torch.as_tensor(o_logits), dim=1).numpy()
    per_board_new_old = np.abs(new[2].reshape(batch, -1) - old[2].reshape(batch, -1)).max(axis=1)
    d_new_old = float(per_board_new_old.max())
    d_old_oracle = float(np.abs(old[2].reshape(batch, -1) - o_logits).max())
    d_new_oracle = float(np.abs(new[2].reshape(batch, -1) - o_logits).max())
    print(name, batch, "logits: quad - tail", d_new_old, "tail - oracle", d_old_oracle, "quad - oracle", d_new_oracle,
          "worst board", int(per_board_new_old.argmax()))
    prob_tol = TOL["prob"]
    if peaked:
        # softmax: |dp_i| <= p_i (|dz_i| + sum_j p_j |dz_j|) <= 2 p_i max |dz|.  max |dz| is taken from the REFERENCE kernel's measured logit
        # deviation (tail - oracle, the figure bound 2 is stated in), not from the allowed 1e-4 and not from the kernel under test; per
        # entry, on top of the parity bound itself: an entry of p = 0.1 may move by 2e-6 + 1e-6 at a logit deviation of 1e-5
        prob_tol = 2 * o_probs * d_old_oracle + TOL["prob"]
    for what, (value, probs, logits, aux) in (("quad", new), ("tail", old)):
        d_probs = np.abs(probs.reshape(batch, -1) - o_probs)
        print(" ", what, "probs - oracle", float(d_probs.max()), "largest oracle probability", float(o_probs.max()),
              "largest bound", float(np.max(prob_tol)))
        assert np.abs(logits.reshape(batch, -1) - o_logits).max() < TOL["logit"], what
        assert np.abs(value - o_value).max() < TOL["value"], what
        assert (d_probs < prob_tol).all(), what
        if cfg.nb_aux:
            assert np.abs(aux.reshape(-1, 4) - o_aux.numpy()).max() < TOL["aux"], what
    assert d_new_old <= d_old_oracle, f"board (= square, in the one-square case) {int(per_board_new_old.argmax())}: {d_new_old} > {d_old_oracle}"


@pytest.mark.parametrize("name,batch", [
    ("risev2-2", 1), ("risev2-2", 3),
    ("risev2-3-plain", 1), ("risev2-3-plain", 3),
    ("risev2-3-gate-first", 3),
    ("risev2-3-gate-mid", 3),
    ("risev33-wdlp", 3),
    ("risev2-19", 8),
])
def test_quadrant_tower_against_the_tail_tower_and_the_oracle(tmp_path, hip_lib, monkeypatch, name, batch):
    _check(tmp_path, monkeypatch, name, batch)


def test_one_changed_square_per_board_every_square_once(tmp_path, hip_lib, monkeypatch):
    cfg, _ = OWN["risev2-3-plain"]()
    # (TOL["prob"] is the parity tests' bound for their boards; these 64 have peaked policies -- a probability of 0.1 moves by 2e-6
    # under a logit error of 1e-5, in either kernel -- so each probability is held to what the tail kernel's measured logit deviation
    # implies for it)
    _check(tmp_path, monkeypatch, "risev2-3-plain", 64, _one_square_boards(cfg.nb_input_channels, 98), peaked=True)
