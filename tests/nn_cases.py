"""Shared NN parity cases: configs, deterministic weights, deterministic inputs (no reference needed at run time)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import rise_oracle as ro  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def small_risev2():
    """3-block RISEv2 parametrisation (C_op 128/192/256), ca_se on the last two blocks, crazyhouse v1 planes."""
    cfg = ro.rise_v2_config(3, 34, 81)
    cfg.se_types = [None, "ca_se", "ca_se"]
    cfg.name = "risev2-3"
    return cfg


def small_risev2_flat():
    cfg = small_risev2()
    cfg.select_policy_from_plane = False
    cfg.n_labels = 2272
    cfg.name = "risev2-3-flat"
    return cfg


CASES = {
    # name: (config factory, seed, stress-init, batch)
    "risev2-3": (small_risev2, 11, True, 4),
    "risev2-7": (lambda: ro.rise_v2_config(7, 34, 81), 12, True, 8),            # BASELINE config 1
    "risev2-13": (lambda: ro.rise_v2_config(13, 34, 81), 13, True, 4),          # the reference's named RISEv2
    "risev2-19": (lambda: ro.rise_v2_config(19, 34, 81), 14, True, 4),          # BASELINE config 2 (headline)
    "risev2-13-default-init": (lambda: ro.rise_v2_config(13, 34, 81), 15, False, 4),
    "risev33": (lambda: ro.rise_v33_config(52, 76, False), 16, True, 4),        # BASELINE config 3
    "risev33-wdlp": (lambda: ro.rise_v33_config(52, 76, True), 17, True, 4),    # released ClassicAra head
    "risev2-13-lichess": (lambda: ro.rise_v2_config(13, 80, 84), 18, True, 2),  # MultiAra tables (config 5)
    # dense 3x3 siblings of the same zoo
    "rise-classical-4": (lambda: ro.rise_classical_config(4, 34, 81), 19, True, 4),
    "alphazero-5": (lambda: ro.alpha_zero_config(5, 52, 76, 4), 20, True, 4),
    "alphazero-3-cv8": (lambda: ro.alpha_zero_config(3, 34, 81, 8), 21, True, 3),
    # SE gates inside the dense blocks: on the block input with hard-sigmoid (ClassicalResidualBlock(se_type)), on the body output with
    # plain sigmoid (AlphaZero ResidualBlock(use_se))
    "rise-classical-3-se": (lambda: ro.rise_classical_config(3, 34, 81, se_types=[None, "ca_se", "eca_se"]), 23, True, 4),
    "alphazero-3-se": (lambda: ro.alpha_zero_config(3, 34, 81, 4, use_se=True), 24, True, 4),
    # flat-label policy head (select_policy_from_plane=False): Linear(P*64 -> 2272 crazyhouse labels)
    "risev2-3-flat": (small_risev2_flat, 22, True, 5),
}


def make_case(name):
    factory, seed, stress, batch = CASES[name]
    cfg = factory()
    sd = ro.make_state_dict(cfg, seed=seed, stress=stress)
    x = synthetic_planes(batch, cfg.nb_input_channels, seed + 1000)
    return cfg, sd, x


def scale_activations(cfg, sd, act=8.0):
    """A copy of `sd` whose activations -- stem output, every tensor of the bottleneck blocks, the heads' hidden layers -- and policy
    logits are `act` times larger (trained nets have logits of +-10 and more; the seeded random nets sit at +-2): the stem's BatchNorm scales
    its output, every later BatchNorm takes running_mean * act and bias * act (BN(act u) with those = act BN(u)), the value head's last
    Linear is divided by `act` so that the value does not saturate.  SE gates see larger means (not homogeneous): a different net, not a
    rescaling of the same function -- a stress case for the precision modes' ABSOLUTE error bounds."""
    out = {k: v.clone() for k, v in sd.items()}
    pre = cfg.key_prefix
    for k in (pre + ".0.body.1.weight", pre + ".0.body.1.bias"):
        out[k] = out[k] * act
    for k in list(out):
        if k.startswith(pre + ".0.body.1."):
            continue
        if k.endswith(".running_mean") or (k.endswith(".bias") and k[:-5] + ".running_mean" in out):
            out[k] = out[k] * act
    out["value_head.body_final.0.bias"] = out["value_head.body_final.0.bias"] * act
    out["value_head.body_final.2.weight"] = out["value_head.body_final.2.weight"] / act
    for k in ("value_head.body_wdl.0.weight", "value_head.body_plys.0.weight"):
        if k in out:
            out[k] = out[k] / act
    return out


def synthetic_planes(batch, channels, seed):
    """Board-like planes: ~88 % zeros, sparse ones, a few constant planes with fractional values."""
    rng = np.random.default_rng(seed)
    x = (rng.random((batch, channels, 8, 8)) < 0.10).astype(np.float32)
    for b in range(batch):
        for c in rng.choice(channels, size=max(2, channels // 8), replace=False):
            x[b, c] = rng.choice([0.0, 1.0, 0.25, 1.0 / 32, 3.0 / 8, 0.002 * (b + 1)])
    return torch.from_numpy(x)


def export_case(tmpdir, name, cfg, sd, version="1.0"):
    from crazyara_amd import netfile
    d = os.path.join(str(tmpdir), name)
    os.makedirs(d, exist_ok=True)
    netfile.export_rise(os.path.join(d, f"{cfg.name}-v{version}.cranet"), cfg, sd, input_version=version)
    return d


# --------------------------------------------------------------------------------------------------------------
# Trained-net-like weights and edge boards (tests/test_trained_like.py, tests/test_trained_like_gpu.py).  make_state_dict(stress=True)
# gives positive BatchNorm gammas, variances of 0.6 ... 1.6, channels that are all O(1), near-uniform policies and values far from
# +-1; trained nets have none of that.  trained_like() moves a seeded net into those regimes.
# --------------------------------------------------------------------------------------------------------------
_NTB_BN_CONV = {"patch_embed.norm": "patch_embed.conv", "projection.norm": "projection.conv", "mhca.norm": "mhca.group_conv3x3"}


def bn_names(sd):
    return [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]


def bn_conv(sd, bn):
    """Key of the conv that feeds BatchNorm `bn`, or None (the NTB pre-norms norm1 / norm2 and the flat head's policy_head.body2.0 get
    no rescaling of a producer: they keep their variance)."""
    head, _, last = bn.rpartition(".")
    if head.endswith(".body") and last.isdigit():
        conv = f"{head}.{int(last) - 1}"
        return conv if conv + ".weight" in sd else None
    for norm, conv in _NTB_BN_CONV.items():
        if bn.endswith("." + norm):
            return bn[:-len(norm)] + conv
    return None


def trained_like(cfg, sd, seed, policy_gain=1.0, value_gain=1.0, spread=32.0, policy_outliers=(0, 1.0)):
    """A copy of `sd` (fp32) in the regimes of a trained net; the arithmetic is done in float64 and rounded once.
      (a) negative gamma on about 25 % of the channels of every BatchNorm;
      (b) about 4 % dead channels (gamma = 0, bias = 0) and 4 % constant channels (gamma = 0, bias kept);
      (c) running_var log-uniform in [1e-4, 4], the producing conv's row and running_mean times sqrt(new / old): the BN output is the
          same up to eps and rounding, the unfolded tensors span 2.5 decades (BNs without a producing conv keep their variance);
      (d) bottleneck blocks: BN1's gamma and bias of channel c times s_c, log-uniform in [1 / spread, spread], depthwise filter c
          divided by s_c (ReLU commutes with s_c > 0: the same function in exact arithmetic, rows of the folded expand weights and
          channels of the expand tile up to spread^2 apart);
      (e) the last policy layer times policy_gain, the last value Linear (the WDL rows) times value_gain.  policy_outliers = (n, K):
          n weights of the last policy layer are first made positive and K times larger.  A gain alone cannot decide a policy: the
          seeded logits of a board are close to Gaussian over the 5184 entries, and a Gaussian of any width has
          max - logsumexp < -1 at that count, i.e. max probability below 0.3 however large the gain (measured: 0.13 ... 0.34 at
          logits of +-23).  A decided policy needs a tail, and a few outlier weights on the post-ReLU hidden planes give one."""
    rng = np.random.default_rng(seed)
    out = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for bn in bn_names(out):
        c = out[bn + ".weight"].numel()
        conv = bn_conv(out, bn)
        if conv is not None:                                                             # (c)
            new = torch.from_numpy(np.exp(rng.uniform(np.log(1e-4), np.log(4.0), c)))
            f = torch.sqrt(new / out[bn + ".running_var"])
            w = out[conv + ".weight"]
            out[conv + ".weight"] = w * f.view(-1, *([1] * (w.dim() - 1)))
            out[bn + ".running_mean"] = out[bn + ".running_mean"] * f
            out[bn + ".running_var"] = new
        u = torch.from_numpy(rng.random(c))
        out[bn + ".weight"] = torch.where(u < 0.25, -out[bn + ".weight"], out[bn + ".weight"])      # (a)
        u = torch.from_numpy(rng.random(c))
        out[bn + ".weight"] = torch.where(u < 0.08, torch.zeros_like(u), out[bn + ".weight"])       # (b): dead and constant
        out[bn + ".bias"] = torch.where(u < 0.04, torch.zeros_like(u), out[bn + ".bias"])           #      dead
    if not cfg.dense_blocks:                                                             # (d)
        for i in range(len(cfg.kernels)):
            p = f"{cfg.key_prefix}.{i + 1}"
            if cfg.transformer(i):
                continue
            c = out[p + ".body.1.weight"].numel()
            s = torch.from_numpy(np.exp(rng.uniform(-np.log(spread), np.log(spread), c)))
            out[p + ".body.1.weight"] = out[p + ".body.1.weight"] * s
            out[p + ".body.1.bias"] = out[p + ".body.1.bias"] * s
            out[p + ".body.3.weight"] = out[p + ".body.3.weight"] / s.view(-1, 1, 1, 1)
    last = ["policy_head.body.3.weight"] if cfg.select_policy_from_plane else ["policy_head.body3.0.weight", "policy_head.body3.0.bias"]
    n_out, k_out = policy_outliers                                                       # (e)
    if n_out:
        w = out[last[0]].reshape(-1).clone()
        idx = torch.from_numpy(rng.choice(w.numel(), n_out, replace=False))
        w[idx] = w[idx].abs() * k_out
        out[last[0]] = w.reshape(out[last[0]].shape)
    for k in last:
        out[k] = out[k] * policy_gain
    head = "value_head.body_wdl.0" if cfg.use_wdl and cfg.use_plys_to_end else "value_head.body_final.2"
    for k in (head + ".weight", head + ".bias"):
        out[k] = out[k] * value_gain
    return {k: (v.float() if v.is_floating_point() else v) for k, v in out.items()}


def edge_planes(x):
    """board 0 all zero, board 1 all one, the last board a copy of board 2, the rest as given (needs at least four boards)"""
    assert x.shape[0] >= 4
    x = x.clone()
    x[0] = 0.0
    x[1] = 1.0
    x[-1] = x[2]
    return x


# name: trained_like()'s arguments and the board count.  The gains were chosen on the CPU against the float64 oracle so that every case
# has a decided and an undecided policy and value and logits inside +-25 (tests/test_trained_like.py asserts it).
TRAINED_LIKE = {
    "risev2-3": dict(seed=10, policy_gain=0.921, value_gain=4.88, policy_outliers=(16, 100.0), batch=4),
    "risev2-7": dict(seed=6, policy_gain=3.36, value_gain=12.0, policy_outliers=(4, 100.0), batch=8),
    "risev33-wdlp": dict(seed=5, policy_gain=6.37, value_gain=15.0, policy_outliers=(16, 100.0), batch=4),
    "risev2-3-flat": dict(seed=6, policy_gain=7.97, value_gain=1.53, policy_outliers=(16, 30.0), batch=5),
    "rise-classical-3-se": dict(seed=5, policy_gain=10.9, value_gain=121.0, policy_outliers=(64, 30.0), batch=4),
    "alphazero-3-se": dict(seed=9, policy_gain=6.71, value_gain=1.79, policy_outliers=(64, 30.0), batch=4),
    "alphazero-3-cv8": dict(seed=31, policy_gain=1.57, value_gain=1.74, policy_outliers=(64, 100.0), batch=4),
    "ntb-224-first-last": dict(seed=19, policy_gain=4.1, value_gain=11.1, policy_outliers=(4, 100.0), batch=5),
}


def seeded_case(name):
    """(cfg, seeded state dict, seeded planes at the trained-like case's board count): CASES, or the reduced NTB net of test_alphavile_gpu"""
    batch = TRAINED_LIKE[name]["batch"]
    if name in CASES:
        factory, seed, stress, _ = CASES[name]
        cfg = factory()
        sd = ro.make_state_dict(cfg, seed=seed, stress=stress)
    else:
        import test_alphavile_gpu
        factory, seed = test_alphavile_gpu.REDUCED[name]
        cfg = factory()
        sd = ro.make_state_dict(cfg, seed=seed)
    return cfg, sd, synthetic_planes(batch, cfg.nb_input_channels, seed + 1000)


def trained_like_case(name):
    """(cfg, trained-like state dict, edge planes)"""
    cfg, sd, x = seeded_case(name)
    args = {k: v for k, v in TRAINED_LIKE[name].items() if k != "batch"}
    return cfg, trained_like(cfg, sd, **args), edge_planes(x)


def oracle_forward(cfg, sd, x):
    """the oracle of the net family, in the dtype of sd"""
    if cfg.has_transformers:
        import alphavile_oracle
        return alphavile_oracle.forward(cfg, sd, x)
    return ro.forward(cfg, sd, x)


_REFERENCE = {}


def trained_like_reference(name):
    """(cfg, sd, x, value, logits, aux) of a trained-like case: the float64 oracle's outputs (numpy float64), computed once per process"""
    if name not in _REFERENCE:
        cfg, sd, x = trained_like_case(name)
        v, l, a = oracle_forward(cfg, ro.to_double(sd), x)
        _REFERENCE[name] = (cfg, sd, x, v.numpy().reshape(-1), l.numpy(), None if a is None else a.numpy())
    return _REFERENCE[name]
