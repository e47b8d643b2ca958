"""GPU: parity of every precision mode on trained-net-like weights and edge boards (nn_cases.trained_like, nn_cases.edge_planes) against
the FLOAT64 oracle (oracle.rise_oracle.to_double): negative, zero and constant BatchNorm channels, variances down to 1e-4, expand
channels 2^10 apart, decided and undecided policies and values, logits up to +-23, an all-zero board, an all-one board and a
duplicated board.

Bounds, copied from tests/test_nn_parity_gpu.py's tables (not imported), with M = max|logit| of the case:
  logits          float32, float16x3 and their suffixed forms: max(1e-4, 4e-5 M), which must itself stay below 1e-3;
                  float16p8: 2.5e-4 M;  float16: 2.2e-3 M (without the 4.8e-3 cap, which was sized for logits of +-2)
  value, aux      1e-4 (float16: 1e-3)
  probabilities   element by element |dp_i| <= 2 p_i L + 2e-7, L = the logit bound: dp_i = p_i (dl_i - sum_j p_j dl_j) gives the first term,
                  the constant is f32 round-off of the exp and the division at p <= 1
  probabilities sum to 1 within 1e-4; every output finite; the duplicated board equals board 2 bit for bit.
A mode runs on the cases where its CPU emulation is within half of these bounds (tests/golden/trained_like_emulation.json, written by
scripts/studies/trained_like_study.py; DESIGN 4 names the cases a mode is not eligible for) and on no others: no case runs with a
widened bound.  fp8 and int8 have no end-to-end bound; they are held block by block, teacher-forced, to the criteria of
tests/test_fp8.py and tests/test_int8.py."""
import json
import os

import numpy as np
import pytest
import torch

import nn_cases
from oracle import rise_oracle as ro

pytestmark = pytest.mark.gpu

VALUE_BOUND = {"float32": 1e-4, "float16x3": 1e-4, "float16p8": 1e-4, "float16": 1e-3}
RISE_MODES = ["float32", "float32-unfused", "float16", "float16-3k", "float16-perblock", "float16-unfused", "float16x3", "float16x3-1wg",
              "float16x3-perblock", "float16x3-unfused", "float16p8", "float16p8-1wg"]
NTB_MODES = ["float32", "float16x3", "float16x3-wblock", "float16x3-wnet", "float16x3-wsplit", "float16x3-wtower"]
DENSE = ("rise-classical-3-se", "alphazero-3-se", "alphazero-3-cv8")
NTB = "ntb-224-first-last"

with open(os.path.join(nn_cases.GOLDEN_DIR, "trained_like_emulation.json")) as _f:
    STUDY = json.load(_f)


def base_mode(precision):
    """the mode whose bounds and emulation a precision string falls under: float16x3-1wg -> float16x3"""
    return max((m for m in list(VALUE_BOUND) + ["fp8", "int8"] if precision == m or precision.startswith(m + "-")), key=len)


def logit_bound(precision, max_logit):
    mode = base_mode(precision)
    if mode in ("float32", "float16x3"):
        bound = max(1e-4, 4e-5 * max_logit)
        assert bound < 1e-3
        return bound
    return {"float16p8": 2.5e-4, "float16": 2.2e-3}[mode] * max_logit


def eligible(name, precision):
    return STUDY[name]["modes"].get(base_mode(precision), {}).get("eligible", False)


def _params():
    out = []
    for name in nn_cases.TRAINED_LIKE:
        modes = NTB_MODES if name == NTB else RISE_MODES + (["float16-2b"] if name in DENSE else [])
        out += [(name, p) for p in modes if eligible(name, p)]
    return out


def _version(cfg):
    return "3.0" if cfg.nb_input_channels in (52, 64, 80) else "1.0"


_runs = {}


def run(tmp_path, name, precision):
    """(value, probabilities, aux, logits) of the case through the C ABI, one net and one forward per (case, precision) of the session"""
    if (name, precision) in _runs:
        return _runs[(name, precision)]
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, x = nn_cases.trained_like_reference(name)[:3]
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version=_version(cfg))
    B = x.shape[0]
    assert 4 <= B <= 8
    net = HipAPI(0, B, d, precision, keep_logits=True)
    value = np.full(B, 7.0, np.float32)
    probs = np.full(B * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(B * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(np.ascontiguousarray(x.numpy()), value, probs, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy()
    net.close()
    _runs[(name, precision)] = (value, probs.reshape(B, -1), None if aux is None else aux.reshape(B, 4), logits)
    return _runs[(name, precision)]


def prob_check(probs, p64, bound, what):
    excess = np.abs(probs - p64) - (2.0 * p64 * bound + 2e-7)
    i = np.unravel_index(int(excess.argmax()), excess.shape)
    assert excess[i] <= 0, (what, i, float(probs[i]), float(p64[i]))


@pytest.mark.parametrize("name,precision", _params())
def test_predict_matches_the_float64_oracle(tmp_path, hip_lib, name, precision):
    cfg, _, x, v64, l64, a64 = nn_cases.trained_like_reference(name)
    value, probs, aux, logits = run(tmp_path, name, precision)
    bound = logit_bound(precision, float(np.abs(l64).max()))
    vbound = VALUE_BOUND[base_mode(precision)]
    p64 = torch.softmax(torch.from_numpy(l64), dim=1).numpy()
    print(f"{name} {precision}: logits {np.abs(logits - l64).max():.3e} (bound {bound:.3e})  value {np.abs(value - v64).max():.3e}  "
          f"probabilities {np.abs(probs - p64).max():.3e}" + ("" if aux is None else f"  aux {np.abs(aux - a64).max():.3e}"))
    assert np.isfinite(value).all() and np.isfinite(probs).all() and np.isfinite(logits).all() and (aux is None or np.isfinite(aux).all())
    for boards in (slice(0, 1), slice(1, 2), slice(None)):              # the all-zero board, the all-one board, all of them
        assert np.abs(logits[boards] - l64[boards]).max() < bound
        assert np.abs(value[boards] - v64[boards]).max() < vbound
        prob_check(probs[boards], p64[boards], bound, precision)
        if aux is not None:
            assert np.abs(aux[boards] - a64[boards]).max() < vbound
    assert np.abs(probs.sum(axis=1) - 1.0).max() < 1e-4
    # the duplicated board
    assert torch.equal(x[-1], x[2])
    assert np.array_equal(logits[-1], logits[2]) and np.array_equal(probs[-1], probs[2]) and value[-1] == value[2]
    assert aux is None or np.array_equal(aux[-1], aux[2])


def test_one_launch_forms_of_the_ntb_net_share_their_bits(tmp_path, hip_lib):
    """what tests/test_x3_wnet_gpu.py and tests/test_x3_wtower_gpu.py say of the seeded nets: -wnet gives -wblock's logits and value,
    -wtower gives every output of -wnet"""
    wblock, wnet, wtower = (run(tmp_path, NTB, "float16x3-" + s) for s in ("wblock", "wnet", "wtower"))
    assert np.array_equal(wblock[3], wnet[3]) and np.array_equal(wblock[0], wnet[0])
    for u, v in zip(wnet, wtower):
        assert (u is None and v is None) or np.array_equal(u, v)


# ---- fp8 and int8: block by block, teacher-forced -----------------------------------------------------------------------------
def _f16_ulp(t):
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _calib_file(d):
    (f,) = [os.path.join(d, n) for n in os.listdir(d) if n.endswith(".int8calib")]
    lines = open(f).read().split("\n")
    return [tuple(float(v) for v in lines[3 + i].split()) for i in range(int(lines[2].split()[1]))]


@pytest.mark.parametrize("name,precision", [(n, p) for n in ("risev2-3", "risev2-7", "risev2-3-flat") for p in ("fp8", "int8") if eligible(n, p)])
def test_8bit_towers_block_by_block_teacher_forced(tmp_path, hip_lib, name, precision):
    """tests/test_fp8.py::test_fp8_tower_block_by_block_teacher_forced and tests/test_int8.py::test_int8_tower_block_by_block_teacher_forced
    on the trained-like nets and the edge boards, each by its own criterion: block i emulated from the kernel's own input of block i
    (oracle.fp8_block / int8_block) against the kernel's output of block i, relative to that block's mode error.  Constant channels
    (BatchNorm gamma = 0, bias != 0) are the rows whose int8 accumulator unit comes from the bias (pack_tower_block)."""
    from crazyara_amd.neuralnetapi import HipAPI, calibrate_int8
    cfg, sd, x = nn_cases.trained_like_reference(name)[:3]
    batch = x.shape[0]
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version=_version(cfg))
    if precision == "int8":
        calibrate_int8(d, 0, nn_cases.synthetic_planes(40, cfg.nb_input_channels, 555).numpy())
        steps = ro.int8_steps(_calib_file(d))
    net = HipAPI(0, batch, d, precision)
    dump = net.block_dump()
    v, p = np.zeros(batch, np.float32), np.zeros(batch * cfg.nb_policy, np.float32)
    net.predict(np.ascontiguousarray(x.numpy()), v, p)
    tiles = torch.as_tensor(dump, device="cuda").cpu().float()                  # [blocks + 1][B][64 squares][256 channels]
    net.close()
    assert tiles.shape[0] == len(cfg.kernels) + 1 and torch.isfinite(tiles).all()
    assert np.isfinite(v).all() and np.isfinite(p).all()
    nchw = lambda t: t.permute(0, 2, 1).reshape(batch, 256, 8, 8).contiguous()
    rows = []
    for i in range(len(cfg.kernels)):
        h_in, h_gpu = nchw(tiles[i]), nchw(tiles[i + 1])
        if precision == "fp8":
            h_emu = ro.fp8_block(cfg, sd, i, h_in, se_f16_weights=True)
        else:
            h_emu = ro.int8_block(cfg, sd, i, h_in, steps[i][0], steps[i][1], se_f16_weights=True)
        err_mode = h_emu - ro.fp32_block(cfg, sd, i, h_in)
        mode_max, mode_rms = float(err_mode.abs().max()), float(err_mode.pow(2).mean().sqrt())
        diff = h_gpu - h_emu
        rows.append((i, float((diff.abs() - _f16_ulp(h_emu)).max()) / mode_max, float(diff.pow(2).mean().sqrt()) / mode_rms,
                     float((diff != 0).float().mean()), mode_max))
    print(f"{name} {precision}: (|gpu - emulation| - ulp) / block mode error: "
          + "; ".join(f"b{i}: max {a:.2f} rms {b:.3f} differ {c:.3f} mode {m:.2e}" for i, a, b, c, m in rows))
    for i, mx, rms, differ, mode_max in rows:
        assert mode_max > (1e-3 if precision == "fp8" else 1e-4), (i, mode_max)
        assert mx <= 0.5 and rms <= 0.1 and differ < (0.5 if precision == "fp8" else 0.25), (name, i, mx, rms, differ)


# ---- gathered priors ----------------------------------------------------------------------------------------------------------
def test_gathered_priors_of_a_decided_policy(tmp_path, hip_lib):
    """mi_net_submit_boards_gathered on the trained-like risev2-7 at batch 8 (descriptors in, planes built on the GPU): the gathered
    entries are the whole vector's probabilities bit for bit, and the entry of the board whose policy is decided (max probability > 0.5)
    is within the probability bound of the float64 oracle.  Boards come from descriptors, so the gain is sized on these eight positions."""
    import experts_cases
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd0, _ = nn_cases.seeded_case("risev2-7")
    sd = nn_cases.trained_like(cfg, sd0, seed=6, policy_gain=5.87, value_gain=12.0, policy_outliers=(16, 100.0))
    playout = experts_cases.playout_positions("crazyhouse", 3, 3, 80)
    positions = playout[:7] + [playout[91]]
    planes = torch.from_numpy(np.stack([p.planes(0, 1, True) for p in positions]).astype(np.float32))
    _, l64, _ = ro.forward(cfg, ro.to_double(sd), planes)
    p64 = torch.softmax(l64, dim=1).numpy()
    assert np.abs(l64.numpy()).max() <= 25.0 and p64[7].max() > 0.5 and p64[:7].max() < 0.5
    top = p64.argmax(axis=1)
    d = nn_cases.export_case(tmp_path, "risev2-7", cfg, sd)
    net = HipAPI(0, 8, d, "float16x3")
    buf = experts_cases.CallBuffers(8, cfg.nb_policy, 96, 0, 0, 0)
    buf.load(positions)
    for s in range(8):                                  # every board's most probable entry is gathered, legal move or not
        n = int(buf.cnt[s])
        if int(top[s]) not in buf.idx[s * 96:s * 96 + n].tolist():
            assert n < 96
            buf.idx[s * 96 + n] = top[s]
            buf.cnt[s] = n + 1
    buf.poison()
    buf.submit_boards(net, 8)
    whole = buf.probs.reshape(8, -1).copy()
    buf.poison()
    buf.submit_gathered(net, 8)
    gathered = buf.gathered.reshape(8, 96).copy()
    lists = [buf.idx[s * 96:s * 96 + int(buf.cnt[s])].astype(np.int64) for s in range(8)]
    buf.close()
    net.close()
    bound = logit_bound("float16x3", float(np.abs(l64.numpy()).max()))
    for s in range(8):
        ids = lists[s]
        assert np.array_equal(gathered[s, :len(ids)], whole[s, ids]), s
        prob_check(gathered[s, :len(ids)], p64[s, ids], bound, s)
        j = ids.tolist().index(int(top[s]))
        assert abs(gathered[s, j] - p64[s, top[s]]) <= 2.0 * p64[s, top[s]] * bound + 2e-7
    prob_check(whole, p64, bound, "whole vectors")
