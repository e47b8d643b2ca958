"""GPU: AlphaVile nets loaded from ONNX model directories (the reference's deployment format) -- the golden cases through mi_net_create
from directories that hold only a .onnx file (tests/alphavile_onnx_writer.py, pinned to torch's exporter by tests/test_onnx_alphavile.py),
the same net from .onnx and from export_rise's .cranet, the .onnx against its own mi_onnx_to_cranet output, and HipAPI behind the
reference's NeuralNetAPI.  Bounds are tests/test_alphavile_gpu.py's (its `check`)."""
import glob
import os

import numpy as np
import pytest
import torch

import alphavile_oracle as ao
import alphavile_onnx_writer as AW
import nn_cases
from test_alphavile_gpu import check

pytestmark = pytest.mark.gpu


def onnx_dir(tmp_path, name, cfg, sd, batch=None, dirname="model"):
    """a model directory holding only the writer's .onnx: '<name>-v3.0.onnx' (dynamic batch) or '<name>-v3.0-bsize-<B>.onnx'"""
    d = os.path.join(str(tmp_path), dirname)
    os.makedirs(d, exist_ok=True)
    fname = f"{cfg.name}-v3.0" + (f"-bsize-{batch}" if batch else "") + ".onnx"
    with open(os.path.join(d, fname), "wb") as f:
        f.write(AW.alpha_vile_to_onnx(cfg, sd, batch=batch))
    return d


def run(d, cfg, x, precision, ops=False):
    from crazyara_amd.neuralnetapi import HipAPI
    B = x.shape[0]
    net = HipAPI(0, B, d, precision, keep_logits=True)
    assert net.get_nb_policy_values() == cfg.nb_policy and net.get_nb_auxiliary_outputs() == cfg.nb_aux
    value = np.full(B, 7.0, np.float32)
    probs = np.full(B * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(B * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(np.ascontiguousarray(x.numpy()), value, probs, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy()
    names = [n for n, _ in net.time_ops(1)] if ops else None
    net.close()
    return (value, probs.reshape(B, -1), aux, logits), names


@pytest.mark.parametrize("precision", ["float32", "float16x3", "float16"])
@pytest.mark.parametrize("batch", [None, 4])
@pytest.mark.parametrize("name", list(ao.CASES))
def test_onnx_directory_matches_golden_and_restatement(tmp_path, hip_lib, name, batch, precision):
    cfg, sd, x = ao.make_case(name)
    g = np.load(nn_cases.GOLDEN_DIR + f"/nn_{name}.npz")
    np.testing.assert_array_equal(g["x"], x.numpy())
    d = onnx_dir(tmp_path, name, cfg, sd, batch)
    outs, _ = run(d, cfg, x, precision)
    check(precision, cfg, sd, x, *outs, golden=g)


@pytest.mark.parametrize("name", list(ao.CASES))
def test_onnx_and_export_rise_give_the_same_net(tmp_path, hip_lib, name):
    """float32 logits within 1e-5 and the same op list: the importer's header builds what export_rise's builds"""
    cfg, sd, x = ao.make_case(name)
    a, ops_a = run(onnx_dir(tmp_path, name, cfg, sd), cfg, x, "float32", ops=True)
    b, ops_b = run(nn_cases.export_case(tmp_path, "cranet", cfg, sd, version="3.0"), cfg, x, "float32", ops=True)
    assert ops_a == ops_b
    assert np.abs(a[3] - b[3]).max() < 1e-5
    assert np.abs(a[0] - b[0]).max() < 1e-5


@pytest.mark.parametrize("precision", ["float32", "float16x3"])
def test_onnx_and_its_own_cranet_are_bit_identical(tmp_path, hip_lib, precision):
    from crazyara_amd import netfile
    cfg, sd, x = ao.make_case("alphavile-normal-wdlp")
    d = onnx_dir(tmp_path, "alphavile-normal-wdlp", cfg, sd, batch=4)
    (src,) = glob.glob(d + "/*.onnx")
    d2 = os.path.join(str(tmp_path), "converted")
    os.makedirs(d2)
    netfile.onnx_to_cranet(src, os.path.join(d2, os.path.basename(src)[:-len(".onnx")] + ".cranet"))
    a, _ = run(d, cfg, x, precision)
    b, _ = run(d2, cfg, x, precision)
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


def test_hipapi_behind_the_reference_base_class_with_an_onnx_directory(tmp_path, hip_lib):
    """integration/hipapi.h through the reference's NeuralNetAPI (oracle/_ref, as tests/test_hipapi_shim_gpu.py) on an ONNX-only
    AlphaVile directory: the base class picks the .onnx and predicts what the restatement does"""
    from oracle import ref_mcts
    if not ref_mcts.hip_available():
        pytest.skip("oracle/_ref/libcrazyara_ref_hip.so not built")
    cfg, sd, x = ao.make_case("alphavile-tiny")
    d = onnx_dir(tmp_path, "alphavile-tiny", cfg, sd, dirname="alphavile")
    B = x.shape[0]
    net = ref_mcts.RefHipAPI(d, 0, B, "float32", 1)
    assert net.model_name().endswith("-v3.0.onnx")
    info = net.info()
    assert info["nb_policy_values"] == cfg.nb_policy and info["batch_size"] == B
    assert net.validate() == 0
    value, probs, _, _ = net.run_inference(x.numpy(), iterations=2)
    net.close()
    o_value, o_logits, _ = ao.forward(cfg, sd, x)
    assert np.abs(value - o_value.numpy().reshape(-1)).max() < 1e-4
    assert np.abs(probs - torch.softmax(o_logits, 1).numpy()).max() < 1e-6
