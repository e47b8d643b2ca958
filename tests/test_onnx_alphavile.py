"""ONNX import of AlphaVile nets (RiseV3 with NextViT transformer blocks), host only: csrc/nn/onnx_import.cpp through mi_onnx_to_cranet.

Pinned two ways, as tests/test_onnx_import.py pins the other families:
  * `reference`: the reference's own module, after merge_bn(), serialised by torch's exporter into tmp_path (the file a CrazyAra user
    holds); the import is checked against the loader-side fold of the un-merged state dict, against the reference module's outputs,
    and the exporter's graph against tests/alphavile_onnx_writer.py op for op (which pins the writer the GPU tests load);
  * always: every flavour of the writer imports to the same tensors, and every graph the importer must refuse names its reason.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import alphavile_oracle as ao
import alphavile_onnx_writer as AW
import nn_cases
from crazyara_amd import netfile, rise_config as rc
from test_alphavile_gpu import REDUCED

BN_EPS = 1e-5
# the golden tiny net and the reduced NTB cases of tests/test_alphavile_gpu.py (M = 32 with eca_se; M = 64 with an NTB first and last)
NAMES = ["alphavile-tiny", "ntb-128-eca", "ntb-224-first-last"]


@pytest.fixture(scope="module")
def lib(hip_lib):
    return hip_lib


def make(name):
    """(cfg, un-merged state dict) of a golden case or a reduced case"""
    if name in ao.CASES:
        cfg, sd, _ = ao.make_case(name)
        return cfg, sd
    factory, seed = REDUCED[name]
    cfg = factory()
    return cfg, rc.make_state_dict(cfg, seed=seed)


def convert(tmp_path, data, fname):
    src = os.path.join(str(tmp_path), fname)
    with open(src, "wb") as f:
        f.write(data)
    return netfile.read_cranet(netfile.onnx_to_cranet(src))


# ---- what the import must produce ---------------------------------------------------------------------------------------------
def _np(sd):
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float64) for k, v in sd.items()}


def _fold(t, conv, bn):
    w = t[conv + ".weight"]
    if bn is None:
        return w, np.zeros(w.shape[0])
    g, b, m, v = (t[f"{bn}.{s}"] for s in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + BN_EPS)
    return w * s.reshape(-1, *([1] * (w.ndim - 1))), b - m * s


def _fold_pre(t, layer, bn):
    """merge_pre_bn as the loader's fold_ntb applies it: W BN(x) + b, W [out][in]"""
    w = t[layer + ".weight"].reshape(t[layer + ".weight"].shape[0], -1)
    g, b, m, v = (t[f"{bn}.{s}"] for s in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + BN_EPS)
    return w * s[None, :], t[layer + ".bias"] + w @ (b - m * s)


def _close(a, b, rtol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= rtol * max(1.0, np.abs(b).max()), (what, err)


def expected_meta(tmp_path, cfg, sd):
    """export_rise's header for the net: the loader must build the same op list from the imported file"""
    meta, _ = netfile.read_cranet(netfile.export_rise(str(tmp_path / "expected.cranet"), cfg, sd, input_version="3.0"))
    return meta


def check_import(tmp_path, cfg, sd, meta, tensors, rtol=1e-6):
    exp = expected_meta(tmp_path, cfg, sd)
    ntb = [cfg.transformer(i) for i in range(len(cfg.kernels))]
    for k in ("nb_input_channels", "channels", "se_types", "channels_value_head", "channels_policy_head", "use_wdl", "use_plys_to_end",
              "conv_block", "select_policy_from_plane", "use_transformers"):
        assert meta[k] == exp[k], (k, meta[k], exp[k])
    if not cfg.use_wdl:
        assert meta["value_fc_size"] == exp["value_fc_size"]
    H = rc.ntb_widths(cfg.channels)[2]
    # an NTB's kernels / channels_operating entries: 3 and the Mlp width (the loader reads them only to size its scratch tiles)
    for key, ntb_value in (("kernels", "3"), ("channels_operating", str(H))):
        got, want = meta[key].split(","), exp[key].split(",")
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == (ntb_value if ntb[i] else w), (key, i, g, w)
    t, s = _np(tensors), _np(sd)
    seen = set()

    def pair(conv, bn):
        for a, b, part in zip(_fold(t, conv, bn), _fold(s, conv, bn), ("weight", "bias")):
            _close(a, b, rtol, f"{conv} folded {part}")
        seen.add(conv + ".weight")
        if bn:
            seen.update(f"{bn}.{x}" for x in ("weight", "bias", "running_mean", "running_var"))

    def exact(name):
        _close(t[name], s[name], rtol, name)
        seen.add(name)

    pair("body_spatial.0.body.0", "body_spatial.0.body.1")
    for i, se in enumerate(cfg.se_types):
        p = f"body_spatial.{i + 1}"
        if ntb[i]:
            pair(p + ".patch_embed.conv", p + ".patch_embed.norm")
            pair(p + ".projection.conv", p + ".projection.norm")
            pair(p + ".mhca.group_conv3x3", p + ".mhca.norm")
            for layer, bn in [(f"{p}.e_mhsa.{n}", p + ".norm1") for n in "qkv"] + [(p + ".mlp.conv1", p + ".norm2")]:
                for a, b, part in zip(_fold_pre(t, layer, bn), _fold_pre(s, layer, bn), ("weight", "bias")):
                    _close(a, b, rtol, f"{layer} with {bn}: {part}")
                seen.update([layer + ".weight", layer + ".bias"] + [f"{bn}.{x}" for x in ("weight", "bias", "running_mean", "running_var")])
            for name in ("e_mhsa.proj.weight", "e_mhsa.proj.bias", "mhca.projection.weight", "mlp.conv2.weight", "mlp.conv2.bias"):
                exact(f"{p}.{name}")
            continue
        if se == "eca_se":
            exact(p + ".se.body.0.weight")
            exact(p + ".se.body.0.bias")
        for c, bn in ((".body.0", ".body.1"), (".body.3", ".body.4"), (".body.6", ".body.7")):
            pair(p + c, p + bn)
    pair("policy_head.body.0", "policy_head.body.1")
    pair("policy_head.body.3", None)
    pair("value_head.body.0", "value_head.body.1")
    heads = ["body_wdl.0", "body_plys.0"] if cfg.use_wdl else ["body_final.0", "body_final.2"]
    for h in heads:
        exact(f"value_head.{h}.weight")
        exact(f"value_head.{h}.bias")
    assert seen == set(tensors), set(tensors) ^ seen


# ---- always: the writer's flavours ----------------------------------------------------------------------------------------------
FLAVOURS = {
    "torch-dynamic": dict(),
    "torch-bsize-4": dict(batch=4),
    "simplified": dict(simplified=True),
    "simplified-split-transposes": dict(simplified=True, split_transposes=True),
    "bn-nodes": dict(fold_bn=False, batch=4),
    "div-scale": dict(scale="div"),
    "other-scale": dict(scale=0.25, batch=4),
}


@pytest.mark.parametrize("name", NAMES + ["alphavile-normal-wdlp"])
def test_every_flavour_imports_to_the_same_tensors(lib, tmp_path, name):
    cfg, sd = make(name)
    first = None
    for flavour, kw in FLAVOURS.items():
        fname = f"{cfg.name}-v3.0" + (f"-bsize-{kw['batch']}" if "batch" in kw else "") + ".onnx"
        meta, tensors = convert(tmp_path, AW.alpha_vile_to_onnx(cfg, sd, **kw), fname)
        check_import(tmp_path, cfg, sd, meta, tensors)
        if first is None:
            first = (meta, tensors)
            continue
        assert meta == first[0], flavour
        if flavour == "bn-nodes":               # (conv weight and BN kept apart: the same fold, checked by check_import above)
            continue
        for k, v in tensors.items():
            if flavour == "other-scale" and ".e_mhsa.q." in k:      # q carries the scale, folded back: equal to rounding
                _close(v.astype(np.float64), first[1][k].astype(np.float64), 1e-6, k)
            else:
                assert np.array_equal(v, first[1][k]), (flavour, k)


def test_standard_scale_leaves_q_bit_identical(lib, tmp_path):
    """Mul(32^-0.5) and Div(sqrt 32) are what the attention kernel applies itself: q's tensors are the file's, bit for bit"""
    cfg, sd = make("alphavile-tiny")
    mg = AW.merged_ntb({k: v.numpy() for k, v in sd.items()}, "body_spatial.15")
    for scale in ("mul", "div"):
        _, t = convert(tmp_path, AW.alpha_vile_to_onnx(cfg, sd, scale=scale), f"s{scale}-v3.0.onnx")
        assert np.array_equal(t["body_spatial.15.e_mhsa.q.weight"], mg["e_mhsa.q.weight"])
        assert np.array_equal(t["body_spatial.15.e_mhsa.q.bias"], mg["e_mhsa.q.bias"])


def test_imported_net_computes_the_un_merged_nets_function(lib, tmp_path):
    """the .cranet of a writer file, run through the test-side restatement, equals the restatement of the original state dict"""
    for name in ("ntb-224-first-last", "alphavile-tiny"):
        cfg, sd = make(name)
        _, tensors = convert(tmp_path, AW.alpha_vile_to_onnx(cfg, sd, scale=0.5), f"{name}-v3.0.onnx")
        x = nn_cases.synthetic_planes(3, cfg.nb_input_channels, 5)
        got = ao.forward(cfg, {k: torch.from_numpy(np.array(v)) for k, v in tensors.items()}, x)
        want = ao.forward(cfg, sd, x)
        for a, b in zip(got, want):
            if b is not None:
                assert float((a - b).abs().max()) < 1e-5


REFUSALS = {
    "sr_ratio": "sr_ratio > 1",
    "head_width": "heads of 32 channels",
    "simple": "'simple' NTB",
    "softmax_axis": "Softmax over axis 2",
    "k_not_transposed": "k is not transposed against q",
    "qk_order": "operands in the wrong order",
    "hard_swish": "hard-swish",
    "concat_order": "E_MHSA part first",
    "mhca_bias": "mhca.projection has a bias",
}


@pytest.mark.parametrize("flaw", AW.FLAWS)
def test_refusals_name_the_block_and_the_reason(lib, tmp_path, flaw):
    cfg, sd = make("ntb-224-first-last")
    for block in (0, 2):                                     # the NTB right behind the stem and the one in front of the heads
        data = AW.alpha_vile_to_onnx(cfg, sd, batch=4, flaw=flaw, flaw_block=block)
        src = os.path.join(str(tmp_path), f"bad-{flaw}-v3.0-bsize-4.onnx")
        with open(src, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError) as e:
            netfile.onnx_to_cranet(src)
        msg = str(e.value)
        assert f"ONNX import: transformer block body_spatial.{block + 1}: " in msg, msg
        assert REFUSALS[flaw] in msg, msg


def test_damaged_transformer_files_raise_and_never_crash(lib, tmp_path):
    """byte damage in a writer file with an NTB (node table first, weights behind it) ends in an error or a valid import"""
    import random
    cfg, sd = make("ntb-128-eca")
    good = [AW.alpha_vile_to_onnx(cfg, sd), AW.alpha_vile_to_onnx(cfg, sd, batch=2, fold_bn=False, split_transposes=True)]
    rng = random.Random(11)
    src, dst = os.path.join(str(tmp_path), "fz-v3.0.onnx"), os.path.join(str(tmp_path), "fz.cranet")
    failed = 0
    for it in range(400):
        b = bytearray(good[it % 2])
        if it % 3 == 0:
            b = b[:rng.randrange(len(b))]
        elif it % 3 == 1:
            for _ in range(rng.randint(1, 3)):
                b[rng.randrange(min(len(b), 20000))] = rng.randrange(256)
        else:
            i = rng.randrange(min(len(b), 20000))
            del b[i:i + rng.randint(1, 48)]
        with open(src, "wb") as f:
            f.write(bytes(b))
        try:
            netfile.onnx_to_cranet(src, dst)
        except ValueError:
            failed += 1
    assert failed > 100


def test_nets_without_transformers_keep_their_header(lib, tmp_path):
    """the importer writes use_transformers only for nets that have an NTB (as export_rise does)"""
    cfg, sd, _ = nn_cases.make_case("risev33-wdlp")
    meta, _ = convert(tmp_path, AW.alpha_vile_to_onnx(cfg, sd), "r-v3.0.onnx")
    assert "use_transformers" not in meta


# ---- reference: torch's exporter on the reference's own module --------------------------------------------------------------------
def reference_module(name, cfg):
    if name in ao.CASES:
        return ao.reference_alpha_vile(ao.CASES[name][0], cfg)
    ao.import_reference_alpha_vile()
    from DeepCrazyhouse.src.domain.neural_net.architectures.pytorch.rise_mobile_v3 import RiseV3
    n = len(cfg.kernels)
    return RiseV3(nb_input_channels=cfg.nb_input_channels, board_height=8, board_width=8, channels=cfg.channels,
                  channels_operating_init=cfg.channels_operating_init, channel_expansion=cfg.channel_expansion, act_types=["relu"] * n,
                  channels_value_head=cfg.channels_value_head, value_fc_size=cfg.value_fc_size, channels_policy_head=cfg.channels_policy_head,
                  dropout_rate=0, select_policy_from_plane=cfg.select_policy_from_plane, kernels=cfg.kernels, se_types=cfg.se_types,
                  use_avg_features=False, n_labels=cfg.n_labels, use_wdl=cfg.use_wdl, use_plys_to_end=cfg.use_plys_to_end,
                  use_mlp_wdl_ply=False, use_transformers=cfg.use_transformers, path_dropout=0,
                  conv_block="mobile_bottlekneck_res_block", kernel_5_channel_ratio=cfg.kernel_5_channel_ratio).eval()


def torch_export(model, cfg, path, batch):
    """trainer_agent_pytorch.py:588-633's export: TorchScript exporter, 'data' in, value / policy (/ aux) out, dynamic or fixed batch.
    The exporter's last step imports the `onnx` package only to splice onnxscript functions in (none here): replaced by the identity,
    as oracle/make_onnx_fixtures.py does."""
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils
    onnx_proto_utils._add_onnxscript_fn = lambda proto, *a, **k: proto
    outputs = ["value_out", "policy_out"] + (["auxiliary_out", "wdl_out", "plys_to_end_out"] if cfg.use_wdl else [])
    x = torch.zeros(batch or 1, cfg.nb_input_channels, 8, 8)
    dyn = None if batch else {n: {0: "batch_size"} for n in ["data"] + outputs}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.onnx.export(model, x, path, input_names=["data"], output_names=outputs, dynamic_axes=dyn, opset_version=20, dynamo=False)
    with open(path, "rb") as f:
        return f.read()


def compute_ops(data):
    """the graph without shape plumbing and views (what the importer matches): op, perm, axis, group, kernel and the shapes of the
    constant inputs, in order"""
    from onnx_reader import read_onnx
    g = read_onnx(data)
    consts = {k: np.asarray(v) for k, v in g.initializers.items()}
    for n in g.nodes:
        if n.op == "Constant" and "value" in n.attrs:
            consts[n.outputs[0]] = np.asarray(n.attrs["value"])
    views = {"Reshape", "Flatten", "Expand", "Squeeze", "Unsqueeze", "Identity", "Dropout", "Cast"}
    shape_valued, out = set(), []
    for n in g.nodes:
        if n.op == "Constant":
            continue
        ins = [i for i in n.inputs if i and i not in consts]
        if n.op == "Shape" or (ins and all(i in shape_valued for i in ins)):
            shape_valued.update(n.outputs)
            continue
        if n.op in views:
            continue
        sig = [n.op] + [f"{k}={list(np.asarray(n.attrs[k]).reshape(-1))}" for k in ("perm", "axis", "group", "kernel_shape") if k in n.attrs]
        sig += [str(tuple(consts[i].shape)) for i in n.inputs if i in consts and consts[i].dtype != np.int64]
        out.append(" ".join(sig))
    return out


@pytest.mark.reference
@pytest.mark.parametrize("batch", [None, 4])
@pytest.mark.parametrize("name", NAMES)
def test_files_of_the_torch_exporter(has_reference, lib, tmp_path, name, batch):
    if not has_reference:
        pytest.skip("/root/reference not present (GPU box)")
    cfg, sd = make(name)
    model = reference_module(name, cfg)
    model.load_state_dict(sd, strict=True)
    x = nn_cases.synthetic_planes(4, cfg.nb_input_channels, 9)
    with torch.no_grad():
        want = model(x)
    model.merge_bn()
    fname = f"{cfg.name}-v3.0" + (f"-bsize-{batch}" if batch else "") + ".onnx"
    data = torch_export(model, cfg, str(tmp_path / fname), batch)
    meta, tensors = netfile.read_cranet(netfile.onnx_to_cranet(str(tmp_path / fname)))
    assert meta["producer"] == "pytorch" and meta["input_version"] == "3.0"
    check_import(tmp_path, cfg, sd, meta, tensors)
    # the imported net computes the reference module's function
    got = ao.forward(cfg, {k: torch.from_numpy(np.array(v)) for k, v in tensors.items()}, x)
    for a, b in zip(got, want):
        assert float((a.reshape(b.shape) - b).abs().max()) < 1e-5
    # the writer the GPU tests load writes this graph, op for op
    assert compute_ops(AW.alpha_vile_to_onnx(cfg, sd, batch=batch)) == compute_ops(data)
