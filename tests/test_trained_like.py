"""Host only: the trained-net-like fixtures (nn_cases.trained_like, nn_cases.edge_planes) are in the regimes they claim, faults in those
regimes are visible in the float64 oracle's logits, the three ways a net reaches the library (container, ONNX with BatchNormalization
nodes, ONNX with folded convolutions) fold BatchNorm to fp32 round-off PER ROW, and the committed emulation study is the one the
study script writes.

The reference everywhere is oracle.rise_oracle.forward / alphavile_oracle.forward on a float64 state dict (rise_oracle.to_double)."""
import json
import os

import numpy as np
import pytest
import torch

import nn_cases
from crazyara_amd import netfile
from oracle import rise_oracle as ro

NAMES = list(nn_cases.TRAINED_LIKE)
BN_EPS = 1e-5


def x3_logit_bound(max_logit):
    """the float16x3 / float32 logit bound of tests/test_trained_like_gpu.py"""
    return max(1e-4, 4e-5 * max_logit)


def _gammas(sd):
    return torch.cat([sd[bn + ".weight"].reshape(-1) for bn in nn_cases.bn_names(sd)])


# ---- regime audit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_trained_like_case_is_in_every_regime(name):
    cfg, sd, x, v, logits, _ = nn_cases.trained_like_reference(name)
    bns = nn_cases.bn_names(sd)
    g = _gammas(sd)
    bias = torch.cat([sd[bn + ".bias"].reshape(-1) for bn in bns])
    # (a) a quarter of the gammas that are left non-zero, in every BatchNorm of 64 channels or more
    assert 0.18 < float((g < 0).float().mean()) < 0.28
    assert all(float((sd[bn + ".weight"] < 0).float().mean()) > 0.1 for bn in bns if sd[bn + ".weight"].numel() >= 64)
    # (b) 4 % dead, 4 % constant
    dead, const = (g == 0) & (bias == 0), (g == 0) & (bias != 0)
    assert 0.025 < float(dead.float().mean()) < 0.055 and 0.025 < float(const.float().mean()) < 0.055
    # (c) every BatchNorm behind a conv: variances over 2.5 decades and more, inside [1e-4, 4]
    for bn in bns:
        var = sd[bn + ".running_var"]
        if nn_cases.bn_conv(sd, bn) is None:
            assert float(var.min()) >= 0.6
            continue
        assert 1e-4 * (1 - 1e-6) <= float(var.min()) and float(var.max()) <= 4.0 * (1 + 1e-6)
        if var.numel() >= 64:
            assert float(var.min()) < 1e-3 and float(var.max()) > 1.0
    # (d) bottleneck blocks: the expand channels' scales two decades apart and more
    for i in range(len(cfg.kernels)):
        if cfg.dense_blocks or cfg.transformer(i):
            continue
        s = (sd[f"{cfg.key_prefix}.{i + 1}.body.1.weight"].abs() / torch.sqrt(sd[f"{cfg.key_prefix}.{i + 1}.body.1.running_var"] + BN_EPS))
        s = s[s > 0]
        assert float(s.max() / s.min()) > 1e3
    # (e) decided and undecided policies and values, logits inside the documented float16x3 range
    p = torch.softmax(torch.from_numpy(logits), dim=1).max(dim=1).values
    assert float(p.max()) > 0.5 and float(p.min()) < 0.05
    assert np.abs(logits).max() <= 25.0
    if not cfg.nb_aux:
        assert np.abs(v).max() > 0.999 and np.abs(v).min() < 0.3
    # edge boards
    assert not x[0].any() and bool((x[1] == 1).all()) and torch.equal(x[-1], x[2])


@pytest.mark.parametrize("name", NAMES)
def test_seeded_case_is_in_none_of_them(name):
    """the table of the fixtures' blind spots as a test: a change of the initialiser that moves the seeded nets shows up here"""
    cfg, sd, x = nn_cases.seeded_case(name)
    g = _gammas(sd)
    assert int((g <= 0).sum()) == 0
    assert min(float(sd[bn + ".running_var"].min()) for bn in nn_cases.bn_names(sd)) >= 0.6
    _, logits, _ = nn_cases.oracle_forward(cfg, ro.to_double(sd), x)
    assert float(torch.softmax(logits, dim=1).max()) < 0.01


# ---- the fixtures see the faults ----------------------------------------------------------------------------------------------
def _abs_gamma(sd):
    return {k: (v.abs() if k[:-len(".weight")] + ".running_var" in sd and k.endswith(".weight") else v) for k, v in sd.items()}


def _drop_constant_bias(sd):
    out = dict(sd)
    for bn in nn_cases.bn_names(sd):
        out[bn + ".bias"] = torch.where(sd[bn + ".weight"] == 0, torch.zeros_like(sd[bn + ".bias"]), sd[bn + ".bias"])
    return out


def _clamp_variance(sd):
    return {k: (v.clamp_min(1e-2) if k.endswith(".running_var") else v) for k, v in sd.items()}


@pytest.mark.parametrize("mutant", [_abs_gamma, _drop_constant_bias, _clamp_variance])
@pytest.mark.parametrize("name", NAMES)
def test_mutants_of_the_oracle_move_the_logits(name, mutant):
    cfg, sd, x, _, logits, _ = nn_cases.trained_like_reference(name)
    _, m_logits, _ = nn_cases.oracle_forward(cfg, mutant(ro.to_double(sd)), x)
    moved = float(np.abs(m_logits.numpy() - logits).max())
    assert moved > 100.0 * x3_logit_bound(float(np.abs(logits).max())), moved


# ---- the float64 path itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["risev2-3", "risev33-wdlp", "alphazero-3-se", "risev2-3-flat"])
def test_default_oracle_path_is_unchanged_and_float64_is_close(name):
    """fp32 state dict: fp32 outputs, the committed golden to fp32 round-off as before; float64 state dict: float64 outputs, and the
    fp32 forward within a few fp32 ulps of max|logit| of them"""
    cfg, sd, x = nn_cases.make_case(name)
    v, l, _ = ro.forward(cfg, sd, x)
    assert v.dtype == torch.float32 and l.dtype == torch.float32
    g = np.load(os.path.join(nn_cases.GOLDEN_DIR, f"nn_{name}.npz"))
    assert np.abs(l.numpy() - g["logits"]).max() < 2e-5
    v64, l64, _ = ro.forward(cfg, ro.to_double(sd), x.double())
    assert v64.dtype == torch.float64 and l64.dtype == torch.float64
    assert float((l.double() - l64).abs().max()) < 2e-6 * float(l64.abs().max())


# ---- folding ------------------------------------------------------------------------------------------------------------------
def _np(sd):
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        k = "body_spatial." + k[len("body."):] if k.startswith("body.") else k
        out[k] = (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float64)
    return out


def _fold(t, conv, bn):
    """(folded weight rows [cout, -1], folded bias, size of the bias' two terms) in float64"""
    w = t[conv + ".weight"]
    w = w.reshape(w.shape[0], -1)
    g, b, m, v = (t[f"{bn}.{s}"] for s in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + BN_EPS)
    return w * s[:, None], b - m * s, np.abs(b) + np.abs(m * s)


def _fold_pre(t, layer, bn):
    """a pre-norm in front of a linear layer: W BN(x) + b"""
    w = t[layer + ".weight"]
    w = w.reshape(w.shape[0], -1)
    g, b, m, v = (t[f"{bn}.{s}"] for s in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + BN_EPS)
    shift = b - m * s
    return w * s[None, :], t[layer + ".bias"] + w @ shift, np.abs(t[layer + ".bias"]) + np.abs(w) @ (np.abs(b) + np.abs(m * s))


def _files(tmp_path, cfg, sd):
    """the net as a container and as the two ONNX flavours, converted by the library's importer: {flavour: tensors}"""
    d = str(tmp_path)
    if cfg.has_transformers:
        import alphavile_onnx_writer
        to_onnx = lambda fold: alphavile_onnx_writer.alpha_vile_to_onnx(cfg, sd, batch=None if not fold else 4, fold_bn=fold)
    else:
        import onnx_writer
        to_onnx = lambda fold: onnx_writer.rise_to_onnx(cfg, sd, batch=None if not fold else 4, fold_bn=fold)
    out = {"cranet": netfile.read_cranet(netfile.export_rise(os.path.join(d, f"{cfg.name}-v3.0.cranet"), cfg, sd, input_version="3.0"))[1]}
    for fold in (False, True):
        os.makedirs(os.path.join(d, f"onnx{int(fold)}"))
        path = os.path.join(d, f"onnx{int(fold)}", f"{cfg.name}-v3.0" + ("-bsize-4" if fold else "") + ".onnx")
        with open(path, "wb") as f:
            f.write(to_onnx(fold))
        out["onnx-folded" if fold else "onnx-bn-nodes"] = netfile.read_cranet(netfile.onnx_to_cranet(path))[1]
    return out


RTOL = 2.0 ** -22       # two fp32 roundings: a fold computed in fp32 from fp32 tensors, or a double fold stored as fp32 and folded again


@pytest.mark.parametrize("name", NAMES)
def test_batchnorm_folds_to_fp32_round_off_per_row(tmp_path, hip_lib, name):
    """Every conv + BatchNorm pair of the three files against the float64 fold of the state dict, row by row: a row of a channel with
    running_var 1e-4 is a hundred times a row with variance 1, and an error that is small against the layer's largest weight can still
    be the whole of a small row.  Rows of dead channels must be exactly zero (weights and bias), rows of constant channels exactly
    zero in the weights.  Tensors that a file keeps unfolded are the state dict's, bit for bit."""
    cfg, sd, _, _, _, _ = nn_cases.trained_like_reference(name)
    src = _np(sd)
    pairs = [(nn_cases.bn_conv(src, bn), bn) for bn in nn_cases.bn_names(src) if nn_cases.bn_conv(src, bn)]
    pre = []
    for i in range(len(cfg.kernels)):
        if cfg.transformer(i):
            p = f"body_spatial.{i + 1}"
            pre += [(f"{p}.e_mhsa.{n}", p + ".norm1") for n in "qkv"] + [(p + ".mlp.conv1", p + ".norm2")]
    if not cfg.select_policy_from_plane:
        pairs.append(("policy_head.body.3", "policy_head.body2.0"))
    assert len(pairs) >= 5
    for flavour, t in _files(tmp_path, cfg, sd).items():
        t = {k: np.asarray(v, np.float64) for k, v in t.items()}
        for fold, todo in ((_fold, pairs), (_fold_pre, pre)):
            for conv, bn in todo:
                w0, b0, bsize = fold(src, conv, bn)
                w1, b1, _ = fold(t, conv, bn)
                assert w1.shape == w0.shape, (flavour, conv)
                rowmax = np.abs(w0).max(axis=1)
                werr = np.abs(w1 - w0).max(axis=1)
                assert (werr <= RTOL * rowmax).all(), (flavour, conv, float((werr / np.maximum(rowmax, 1e-300)).max()))
                assert (np.abs(b1 - b0) <= RTOL * bsize).all(), (flavour, conv, float((np.abs(b1 - b0) / np.maximum(bsize, 1e-300)).max()))
                if fold is _fold:
                    g, b = src[bn + ".weight"], src[bn + ".bias"]
                    assert not w1[g == 0].any(), (flavour, conv)
                    assert not b1[(g == 0) & (b == 0)].any(), (flavour, conv)
                # unfolded tensors: the container holds the state dict; the importer keeps a BatchNormalization node's conv weights and
                # writes the node as scale and shift
                kept = {"cranet": [conv + ".weight"] + [f"{bn}.{s}" for s in ("weight", "bias", "running_mean", "running_var")],
                        "onnx-bn-nodes": [conv + ".weight"] if fold is _fold else [], "onnx-folded": []}[flavour]
                for k in kept:
                    assert np.array_equal(t[k], src[k].reshape(t[k].shape)), (flavour, k)


# ---- mode eligibility ---------------------------------------------------------------------------------------------------------
STUDY = os.path.join(nn_cases.GOLDEN_DIR, "trained_like_emulation.json")


def test_emulation_study_is_committed_and_covers_every_case():
    with open(STUDY) as f:
        study = json.load(f)
    assert sorted(study) == sorted(NAMES)
    for name, rec in study.items():
        assert rec["max_logit"] <= 25.0 and rec["max_prob"] > 0.5
        # float32 and float16x3 run everywhere: their emulations are within half of the bound on every case
        for mode in ("float32", "float16x3"):
            assert rec["modes"][mode]["eligible"], (name, mode)
            assert rec["modes"][mode]["logit_error"] <= 0.5 * x3_logit_bound(rec["max_logit"])
    for mode in ("float16", "float16p8", "fp8", "int8"):
        assert sum(rec["modes"].get(mode, {}).get("eligible", False) for rec in study.values()) >= 3, mode


@pytest.mark.parametrize("name", ["risev2-3", "alphazero-3-cv8", "ntb-224-first-last"])
def test_emulation_study_is_regenerable(name):
    """the study script gives the committed figures (three of the cases; the others take the same path)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("trained_like_study", os.path.join(nn_cases.ROOT, "scripts", "studies", "trained_like_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(STUDY) as f:
        want = json.load(f)[name]
    got = mod.study(name)
    assert got["modes"].keys() == want["modes"].keys()
    assert abs(got["max_logit"] - want["max_logit"]) < 1e-9 * want["max_logit"]
    for mode, w in want["modes"].items():
        assert got["modes"][mode]["eligible"] == w["eligible"], mode
        # (the fp32 emulations sum in an order that depends on the machine's thread count and BLAS: the error's size, not its bits)
        assert 0.5 * w["logit_error"] <= got["modes"][mode]["logit_error"] <= 2.0 * w["logit_error"], mode
