"""RISE network descriptions + deterministic random weights (product side).

Mirrors what the reference's `generate_random_nn.py` provides (DeepCrazyhouse/src/domain/neural_net/generate_random_nn.py:136-165):
a way to obtain a RISEv2 / RISEv3.3 model with seeded random parameters when no trained weights ship
(model/params/README.md).  The constructor fields are those of `RiseV3` (rise_mobile_v3.py:81-120); parameter names
are the reference's state-dict keys so real checkpoints export through crazyara_amd.netfile.export_rise unchanged.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, asdict
from typing import Dict, List, Optional

import numpy as np
import torch


@dataclass
class RiseConfig:
    nb_input_channels: int = 34
    channels: int = 256
    channels_operating_init: int = 128
    channel_expansion: int = 64
    kernels: List[int] = field(default_factory=lambda: [3] * 13)
    se_types: List[Optional[str]] = field(default_factory=lambda: [None] * 13)
    channels_value_head: int = 8
    value_fc_size: int = 256
    channels_policy_head: int = 81
    use_wdl: bool = False
    use_plys_to_end: bool = False
    name: str = "risev2"
    # residual block family:
    #   "mobile_bottlekneck_res_block"  RiseV3 default: 1x1 expand, depthwise kxk, 1x1 project (builder_util.py:437-475)
    #   "classical_res_block"           RiseV3(conv_block=...): x + ReLU(BN(conv3x3(ReLU(BN(conv3x3(x))))))  (builder_util.py:401-434)
    #   "a0_res_block"                  AlphaZeroResnet: ReLU(x + BN(conv3x3(ReLU(BN(conv3x3(x))))))          (a0_resnet.py:72-183)
    conv_block: str = "mobile_bottlekneck_res_block"
    # policy head form (_PolicyHead, builder_util.py:206-243): True = policy map (logits = the P x 8 x 8 planes, channel-major);
    # False = flat labels: BN + ReLU on the planes, then Linear(P*64 -> n_labels)
    select_policy_from_plane: bool = True
    n_labels: int = 2272
    # RiseV3(use_transformers=...): use_transformers[i] makes block i a NextViT transformer block (NTB, next_vit_official_modules.py:267-335)
    # instead of a bottleneck; None = none (AlphaVile nets, alpha_vile.py)
    use_transformers: Optional[List[bool]] = None
    # RiseV3(kernel_5_channel_ratio=...): the 5x5 blocks' C_op is int(C_op * ratio + 0.5) instead of C_op - 32 * (idx // 2)
    kernel_5_channel_ratio: Optional[float] = None

    @property
    def dense_blocks(self) -> bool:
        return self.conv_block in ("classical_res_block", "a0_res_block")

    @property
    def key_prefix(self) -> str:
        """state-dict prefix of stem + blocks: RiseV3.body_spatial, AlphaZeroResnet.body"""
        return "body" if self.conv_block == "a0_res_block" else "body_spatial"

    def channels_operating(self) -> List[int]:
        """C_op per block, rise_mobile_v3.py:36-78 (_get_res_blocks, both kernel_5_channel_ratio branches)."""
        out = []
        c = self.channels_operating_init
        for idx, k in enumerate(self.kernels):
            if k != 5:
                out.append(c)
            elif self.kernel_5_channel_ratio is None:
                out.append(c - 32 * (idx // 2))
            else:
                out.append(int(c * self.kernel_5_channel_ratio + 0.5))
            c += self.channel_expansion
        return out

    def transformer(self, i: int) -> bool:
        return bool(self.use_transformers and self.use_transformers[i])

    @property
    def has_transformers(self) -> bool:
        return any(self.transformer(i) for i in range(len(self.kernels)))

    @property
    def nb_policy(self) -> int:
        return self.channels_policy_head * 64 if self.select_policy_from_plane else self.n_labels

    @property
    def nb_aux(self) -> int:
        return 4 if (self.use_wdl and self.use_plys_to_end) else 0

    def to_dict(self):
        return asdict(self)


def rise_v2_config(n_blocks: int = 13, nb_input_channels: int = 34, channels_policy_head: int = 81) -> RiseConfig:
    """RISEv2 parametrised by block count; ca_se on the last 5 blocks (rise_mobile_v3.py:217-241)."""
    se = [None] * n_blocks
    for i in range(max(0, n_blocks - 5), n_blocks):
        se[i] = "ca_se"
    return RiseConfig(nb_input_channels=nb_input_channels, channels=256, channels_operating_init=128,
                      channel_expansion=64, kernels=[3] * n_blocks, se_types=se,
                      channels_policy_head=channels_policy_head, name=f"risev2-{n_blocks}")


def rise_v33_config(nb_input_channels: int = 52, channels_policy_head: int = 76, wdlp: bool = False) -> RiseConfig:
    """RISEv3.3 (rise_mobile_v3.py:186-214)."""
    kernels = [3] * 15
    for i in (7, 11, 12, 13):
        kernels[i] = 5
    se = [None] * 15
    for i in (5, 8, 12, 13, 14):
        se[i] = "eca_se"
    return RiseConfig(nb_input_channels=nb_input_channels, channels=256, channels_operating_init=224,
                      channel_expansion=32, kernels=kernels, se_types=se,
                      channels_policy_head=channels_policy_head, use_wdl=wdlp, use_plys_to_end=wdlp,
                      name="risev3.3" + ("-wdlp" if wdlp else ""))


def rise_classical_config(n_blocks: int = 19, nb_input_channels: int = 34, channels_policy_head: int = 81,
                          se_types: Optional[List[Optional[str]]] = None) -> RiseConfig:
    """RiseV3(conv_block="classical_res_block"): a tower of dense 3x3 residual blocks (rise_mobile_v3.py:71-72).  se_types[i] gates the
    INPUT of block i (hard-sigmoid), ClassicalResidualBlock.forward, builder_util.py:425-434."""
    return RiseConfig(nb_input_channels=nb_input_channels, channels=256, channels_operating_init=256, channel_expansion=0,
                      kernels=[3] * n_blocks, se_types=list(se_types) if se_types else [None] * n_blocks,
                      channels_policy_head=channels_policy_head,
                      conv_block="classical_res_block", name=f"rise-classical-{n_blocks}" + ("-se" if se_types else ""))


def alpha_zero_config(n_blocks: int = 19, nb_input_channels: int = 34, channels_policy_head: int = 81,
                      channels_value_head: int = 4, use_se: bool = False) -> RiseConfig:
    """AlphaZeroResnet as get_alpha_zero_model builds it (a0_resnet.py:172-183): 19 blocks, value head 4 channels.  use_se: every
    ResidualBlock gates its body OUTPUT with get_se("se", use_hard_sigmoid=False) before the shortcut (a0_resnet.py:94-107)."""
    return RiseConfig(nb_input_channels=nb_input_channels, channels=256, channels_operating_init=256, channel_expansion=0,
                      kernels=[3] * n_blocks, se_types=(["se"] if use_se else [None]) * n_blocks, channels_value_head=channels_value_head,
                      channels_policy_head=channels_policy_head, conv_block="a0_res_block",
                      name=f"alphazero-{n_blocks}" + ("-se" if use_se else ""))


def make_divisible(v, divisor: int = 32) -> int:
    """next_vit_official_modules.py:_make_divisible (min_value = divisor)"""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def ntb_widths(channels: int):
    """NTB(channels, channels) with its defaults (mix_block_ratio 0.75, mlp_ratio 2, head_dim 32): (D, M, hidden) -- the E_MHSA width,
    the MHCA width (channels - D) and the Mlp's hidden width."""
    d = make_divisible(int(channels * 0.75), 32)
    return d, channels - d, make_divisible(channels * 2, 32)


_ALPHA_VILE_K5 = {"tiny": (1, 2, 6, 7, 8, 9, 10), "small": (0, 4, 5, 6, 10, 11, 13, 15, 17, 20),
                  "normal": (0, 4, 5, 7, 10, 12, 15, 16, 20, 21, 22, 23, 24, 25),
                  "large": (1, 6, 7, 9, 10, 14, 18, 19, 23, 25, 26, 27, 28, 29, 33, 34, 35)}


def alpha_vile_config(size: str = "normal", nb_input_channels: int = 52, channels_policy_head: int = 76, wdlp: bool = False) -> RiseConfig:
    """AlphaVile as get_alpha_vile_model builds it (alpha_vile.py:14-158): RiseV3 with mobile bottlenecks, one or two NTBs, no SE."""
    if size not in _ALPHA_VILE_K5:
        raise ValueError(f"unknown AlphaVile size '{size}' (tiny | small | normal | large)")
    channels = {"tiny": 192, "small": 192, "normal": 224, "large": 224}[size]
    depth = {"tiny": 15, "small": 22, "normal": 26, "large": 37}[size]
    nb_transformers = 2 if size in ("normal", "large") else 1
    expansion_ratio = 2
    ratio = (int(((channels * expansion_ratio * 0.68) / 32) + 0.5) * 32) / (channels * expansion_ratio)
    kernels = [3] * depth
    for i in _ALPHA_VILE_K5[size]:
        kernels[i] = 5
    use_transformers = [False] * depth
    block_size = depth // (nb_transformers + 1)
    for idx in range(depth % block_size + 2 * block_size - 1, depth, block_size):
        use_transformers[idx] = True
    return RiseConfig(nb_input_channels=nb_input_channels, channels=channels, channels_operating_init=channels * expansion_ratio,
                      channel_expansion=0, kernels=kernels, se_types=[None] * depth, channels_value_head=8, value_fc_size=channels,
                      channels_policy_head=channels_policy_head, use_wdl=wdlp, use_plys_to_end=wdlp,
                      use_transformers=use_transformers, kernel_5_channel_ratio=ratio,
                      name=f"alphavile-{size}" + ("-wdlp" if wdlp else ""))


def eca_kernel(channels: int, gamma: int = 2, b: int = 1) -> int:
    t = int(abs((math.log(channels, 2) + b) / gamma))
    return t if t % 2 else t + 1


# --------------------------------------------------------------------------------------------------------------
# deterministic weights (numpy PCG64: identical on every machine; the reference has no trained weights in-tree)
# --------------------------------------------------------------------------------------------------------------
def make_state_dict(cfg: RiseConfig, seed: int = 0, stress: bool = True) -> Dict[str, torch.Tensor]:
    """State dict with the reference's key names.

    stress=True : variance-preserving weights + randomised BN statistics so that activations/logits are O(1)
                  (torch's default init makes the residual branches vanish -> a 1e-3 test would be vacuous).
    stress=False: mimic torch default init magnitudes (kaiming-uniform a=sqrt(5)), BN identity stats.
    """
    rng = np.random.default_rng(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, cout, cin_per_group, k, gain=1.0):
        fan_in = cin_per_group * k * k
        if stress:
            std = gain * math.sqrt(2.0 / fan_in)
            w = rng.standard_normal((cout, cin_per_group, k, k)) * std
        else:
            bound = 1.0 / math.sqrt(fan_in)
            w = rng.uniform(-bound, bound, (cout, cin_per_group, k, k))
        sd[name + ".weight"] = torch.tensor(w, dtype=torch.float32)

    def bn(name, c, out_scale=1.0):
        if stress:
            g = rng.uniform(0.6, 1.4, c) * out_scale
            b = rng.normal(0, 0.15, c) * out_scale
            m = rng.normal(0, 0.15, c)
            v = rng.uniform(0.6, 1.6, c)
        else:
            g, b, m, v = np.ones(c), np.zeros(c), np.zeros(c), np.ones(c)
        sd[name + ".weight"] = torch.tensor(g, dtype=torch.float32)
        sd[name + ".bias"] = torch.tensor(b, dtype=torch.float32)
        sd[name + ".running_mean"] = torch.tensor(m, dtype=torch.float32)
        sd[name + ".running_var"] = torch.tensor(v, dtype=torch.float32)
        sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)

    def linear(name, cout, cin, bias=True, gain=1.0):
        if stress:
            w = rng.standard_normal((cout, cin)) * gain * math.sqrt(2.0 / cin)
            b = rng.normal(0, 0.1, cout)
        else:
            bound = 1.0 / math.sqrt(cin)
            w = rng.uniform(-bound, bound, (cout, cin))
            b = rng.uniform(-bound, bound, cout)
        sd[name + ".weight"] = torch.tensor(w, dtype=torch.float32)
        if bias:
            sd[name + ".bias"] = torch.tensor(b, dtype=torch.float32)

    def conv_bias(name, cout, fan_in):
        b = rng.normal(0, 0.1, cout) if stress else rng.uniform(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in), cout)
        sd[name + ".bias"] = torch.tensor(b, dtype=torch.float32)

    def ntb(p, nblk):
        """NTB(C, C) (next_vit_official_modules.py:267-335), sr_ratio 1: the reference's parameter names.  Stress init: q / k at twice
        the variance-preserving scale, so that the softmax over the 64 squares is neither flat nor one-hot; the three branches that add
        into the stream (proj, MHCA projection, mlp.conv2) scaled like a bottleneck's last BN."""
        D, M, H = ntb_widths(C)
        out = (1.0 / math.sqrt(nblk)) if stress else 1.0
        conv(p + ".patch_embed.conv", D, C, 1, gain=0.5)      # (no shortcut around patch_embed: keep the stream's scale)
        bn(p + ".patch_embed.norm", D)
        bn(p + ".norm1", D)
        linear(p + ".e_mhsa.q", D, D, gain=math.sqrt(2.0))
        linear(p + ".e_mhsa.k", D, D, gain=math.sqrt(2.0))
        linear(p + ".e_mhsa.v", D, D)
        linear(p + ".e_mhsa.proj", D, D, gain=out)
        conv(p + ".projection.conv", M, D, 1)
        bn(p + ".projection.norm", M)
        conv(p + ".mhca.group_conv3x3", M, 32, 3)
        bn(p + ".mhca.norm", M)
        conv(p + ".mhca.projection", M, M, 1, gain=out)
        bn(p + ".norm2", C)
        conv(p + ".mlp.conv1", H, C, 1)
        conv_bias(p + ".mlp.conv1", H, C)
        conv(p + ".mlp.conv2", C, H, 1, gain=0.5 * out)
        conv_bias(p + ".mlp.conv2", C, H)

    C = cfg.channels
    pre = cfg.key_prefix
    conv(pre + ".0.body.0", C, cfg.nb_input_channels, 3, gain=2.0)
    bn(pre + ".0.body.1", C)
    nblk = len(cfg.kernels)
    for i, (k, cop, se) in enumerate(zip(cfg.kernels, cfg.channels_operating(), cfg.se_types)):
        p = f"{pre}.{i + 1}"
        if cfg.transformer(i):
            ntb(p, nblk)
            continue
        if cfg.dense_blocks:
            if se in ("ca_se", "se"):
                linear(p + ".se.fc.0", C // 2, C, bias=False)
                linear(p + ".se.fc.2", C, C // 2, bias=False, gain=2.0)
            elif se == "eca_se":
                kk = eca_kernel(C)
                w = rng.standard_normal((C, C, kk)) * (2.0 * math.sqrt(2.0 / C) if stress else 1.0 / math.sqrt(C * kk))
                sd[p + ".se.body.0.weight"] = torch.tensor(w, dtype=torch.float32)
                sd[p + ".se.body.0.bias"] = torch.tensor(rng.normal(0, 0.5 if stress else 0.01, C), dtype=torch.float32)
            conv(p + ".body.0", C, C, 3)
            bn(p + ".body.1", C)
            conv(p + ".body.3", C, C, 3)
            bn(p + ".body.4", C, out_scale=(0.5 / math.sqrt(nblk)) if stress else 1.0)
            continue
        if se in ("ca_se", "se"):
            linear(p + ".se.fc.0", C // 2, C, bias=False)
            linear(p + ".se.fc.2", C, C // 2, bias=False, gain=2.0)
        elif se == "eca_se":
            kk = eca_kernel(C)
            w = rng.standard_normal((C, C, kk)) * (2.0 * math.sqrt(2.0 / C) if stress else 1.0 / math.sqrt(C * kk))
            sd[p + ".se.body.0.weight"] = torch.tensor(w, dtype=torch.float32)
            sd[p + ".se.body.0.bias"] = torch.tensor(rng.normal(0, 0.5 if stress else 0.01, C), dtype=torch.float32)
        conv(p + ".body.0", cop, C, 1)
        bn(p + ".body.1", cop)
        conv(p + ".body.3", cop, 1, k, gain=1.2)
        bn(p + ".body.4", cop)
        conv(p + ".body.6", C, cop, 1)
        # keep the residual stream O(1) over many blocks
        bn(p + ".body.7", C, out_scale=(1.0 / math.sqrt(nblk)) if stress else 1.0)
    conv("policy_head.body.0", C, C, 3)
    bn("policy_head.body.1", C)
    conv("policy_head.body.3", cfg.channels_policy_head, C, 3, gain=0.35 if cfg.dense_blocks or cfg.has_transformers else 1.0)   # logits O(1) either way
    if not cfg.select_policy_from_plane:
        bn("policy_head.body2.0", cfg.channels_policy_head)
        linear("policy_head.body3.0", cfg.n_labels, cfg.channels_policy_head * 64, gain=0.35)
    conv("value_head.body.0", cfg.channels_value_head, C, 1)
    bn("value_head.body.1", cfg.channels_value_head)
    nflat = 64 * cfg.channels_value_head
    # (transformer nets: AlphaVile's deep trunks carry a larger stream into the heads; smaller head gains keep value and WDL logits O(0.3))
    vg = 0.25 if cfg.has_transformers else 1.0
    if cfg.use_wdl:
        linear("value_head.body_wdl.0", 3, nflat, gain=0.7 * vg)
    if cfg.use_plys_to_end:
        linear("value_head.body_plys.0", 1, nflat, gain=0.7 * vg)
    linear("value_head.body_final.0", cfg.value_fc_size, nflat)
    linear("value_head.body_final.2", 1, cfg.value_fc_size, gain=0.5 * vg)
    return sd
