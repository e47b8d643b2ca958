"""GPU: AlphaVile nets (RiseV3 with NextViT transformer blocks) through the C ABI -- predict against the reference goldens and the
test-side restatement (tests/alphavile_oracle.py), reduced NTB cases, determinism, refusals and the search pool.

float32, float16x3 and float16p8 are held to tests/test_nn_parity_gpu.py's bounds (copied, not imported): 1e-4 on logits and value (float16p8:
3e-4 on the logits), 1e-6 on the probabilities.  float16 is NOT held to that file's float16 bounds (value 1e-3, probabilities 1e-5, aux 1e-3,
logits 2.2e-3 x max|logit| capped at 4.8e-3), which were measured on the fused 256-channel nets: on these nets every layer's output is
stored in f16, and the emulation of exactly those roundings on the fp32 forward (alphavile_oracle.forward_f16) already errs by 2.3e-3 x
max|logit| = 9.0e-3 on the logits and 1.0e-3 on the aux outputs of the goldens (tests/test_alphavile.py checks that it exceeds them).
float16 bounds here: value 2e-3 (as test_other_trunk_widths_run_on_the_layer_kernels), logits 3.5e-3 x max|logit| (at most 1e-2),
probabilities 3e-5, aux 2e-3 -- and, per case, the logit error at most 1.5 x that of the emulation plus 1e-3."""
import numpy as np
import pytest
import torch

import alphavile_oracle as ao
import nn_cases
from crazyara_amd import rise_config as rc

pytestmark = pytest.mark.gpu

TOL = {"float32": dict(logit=1e-4, logit_rel=None, value=1e-4, prob=1e-6, aux=1e-4),
       "float16": dict(logit=4.8e-3, logit_rel=2.2e-3, value=1e-3, prob=1e-5, aux=1e-3)}
TOL["float16x3"] = TOL["float32"]
TOL["float16p8"] = dict(logit=3e-4, logit_rel=None, value=1e-4, prob=1e-6, aux=1e-4)
# float16 on the layer path (module docstring): measured on the MI355X 8.8e-3 / 6.3e-3 on the logits of tiny / normal (emulation 9.0e-3 /
# 7.0e-3), 1.35e-3 on the value, 1.8e-5 on the probabilities
TOL["float16-layers"] = dict(logit=1e-2, logit_rel=3.5e-3, value=2e-3, prob=3e-5, aux=2e-3)


def logit_tol(tol, ref_logits):
    if tol["logit_rel"] is None:
        return tol["logit"]
    return min(tol["logit"], max(2e-4, tol["logit_rel"] * float(np.abs(np.asarray(ref_logits)).max())))


def reduced(C, kernels, ntbs, se=None, wdlp=False):
    """a small RiseV3 net of width C with NTBs at the given blocks (AlphaVile's settings otherwise), chess v3.0 planes"""
    n = len(kernels)
    ratio = (int(2 * C * 0.68 / 32 + 0.5) * 32) / (2 * C)          # alpha_vile.py's kernel_5_channel_ratio for width C
    cfg = rc.RiseConfig(nb_input_channels=52, channels=C, channels_operating_init=2 * C, channel_expansion=0, kernels=list(kernels),
                        se_types=list(se) if se else [None] * n, value_fc_size=C, channels_policy_head=76, use_wdl=wdlp,
                        use_plys_to_end=wdlp, use_transformers=[i in ntbs for i in range(n)], kernel_5_channel_ratio=ratio,
                        name=f"ntb-{C}")
    return cfg


REDUCED = {
    # M = 32 (one MHCA group), an eca_se block right behind the NTB
    "ntb-128-eca": (lambda: reduced(128, [3, 5, 3], [1], se=[None, None, "eca_se"]), 41),
    # M = 64 (two groups), an NTB as the first block and as the last (the heads read it)
    "ntb-224-first-last": (lambda: reduced(224, [3, 5, 3], [0, 2]), 42),
    # a plain 224-channel RISE net: every kernel of the layer path at 224
    "plain-224": (lambda: rc.RiseConfig(nb_input_channels=52, channels=224, channels_operating_init=448, channel_expansion=0,
                                        kernels=[3, 5, 3], se_types=[None, None, "eca_se"], value_fc_size=224, channels_policy_head=76,
                                        kernel_5_channel_ratio=0.7142857142857143, name="plain-224"), 43),
}


def run(tmp_path, cfg, sd, x, precision, name):
    from crazyara_amd.neuralnetapi import HipAPI
    d = nn_cases.export_case(tmp_path, name, cfg, sd, version="3.0")
    B = x.shape[0]
    net = HipAPI(0, B, d, precision, keep_logits=True)
    assert net.get_nb_policy_values() == cfg.nb_policy and net.get_nb_auxiliary_outputs() == cfg.nb_aux
    assert abs(net.flops_per_position() - ao.flops_per_position(cfg)) < 1.0
    value = np.full(B, 7.0, np.float32)
    probs = np.full(B * cfg.nb_policy, 7.0, np.float32)
    aux = np.full(B * 4, 7.0, np.float32) if cfg.nb_aux else None
    net.predict(np.ascontiguousarray(x.numpy()), value, probs, aux)
    logits = torch.as_tensor(net.device_buffers()["logits"], device="cuda").cpu().numpy()
    net.close()
    return value, probs.reshape(B, -1), aux, logits


def check(precision, cfg, sd, x, value, probs, aux, logits, golden=None):
    tol = TOL["float16-layers" if precision == "float16" else precision]
    o_value, o_logits, o_aux = ao.forward(cfg, sd, x)
    refs = [(o_value.numpy().reshape(-1), o_logits.numpy(), None if o_aux is None else o_aux.numpy())]
    if golden is not None:
        refs.append((golden["value"], golden["logits"], golden["aux"] if "aux" in golden else None))
    for ref_v, ref_l, ref_a in refs:
        assert np.abs(value - ref_v).max() < tol["value"]
        assert np.abs(logits - ref_l).max() < logit_tol(tol, ref_l)
        if ref_a is not None:
            assert np.abs(aux.reshape(-1, 4) - ref_a).max() < tol["aux"]
    assert np.abs(probs - torch.softmax(o_logits, dim=1).numpy()).max() < tol["prob"]
    if precision == "float16":          # no worse than what f16 storage alone explains on this net
        e_logits = ao.forward_f16(cfg, sd, x)[1].numpy()
        emulated = float(np.abs(e_logits - o_logits.numpy()).max())
        measured = float(np.abs(logits - o_logits.numpy()).max())
        print(f"float16 logits: measured {measured:.2e}, emulated f16 storage {emulated:.2e}, GPU - emulation {np.abs(logits - e_logits).max():.2e}")
        assert measured < 1.5 * emulated + 1e-3


@pytest.mark.parametrize("precision", ["float32", "float16x3", "float16", "float16p8"])
@pytest.mark.parametrize("name", list(ao.CASES))
def test_predict_matches_golden_and_restatement(tmp_path, hip_lib, name, precision):
    cfg, sd, x = ao.make_case(name)
    g = np.load(nn_cases.GOLDEN_DIR + f"/nn_{name}.npz")
    np.testing.assert_array_equal(g["x"], x.numpy())
    check(precision, cfg, sd, x, *run(tmp_path, cfg, sd, x, precision, name), golden=g)


@pytest.mark.parametrize("precision,batch", [("float16x3", 1), ("float16x3", 5), ("float16x3", 256), ("float32", 5), ("float16", 5),
                                             ("float32", 256)])
def test_batch_sizes(tmp_path, hip_lib, precision, batch):
    cfg, sd, _ = ao.make_case("alphavile-tiny")
    x = nn_cases.synthetic_planes(batch, 52, 500 + batch)
    check(precision, cfg, sd, x, *run(tmp_path, cfg, sd, x, precision, "alphavile-tiny"))


@pytest.mark.parametrize("precision", ["float32", "float16x3", "float16"])
@pytest.mark.parametrize("name", list(REDUCED))
def test_reduced_ntb_cases(tmp_path, hip_lib, name, precision):
    factory, seed = REDUCED[name]
    cfg = factory()
    sd = rc.make_state_dict(cfg, seed=seed)
    if not cfg.has_transformers:        # (the plain net's seeded logits reach +-5.8; halved, like the transformer nets' policy head gain)
        sd["policy_head.body.3.weight"] = sd["policy_head.body.3.weight"] * 0.5
    x = nn_cases.synthetic_planes(5, 52, seed)
    check(precision, cfg, sd, x, *run(tmp_path, cfg, sd, x, precision, name))


@pytest.mark.parametrize("precision", ["float32", "float16x3", "float16"])
def test_two_runs_and_poisoned_lds_give_identical_bits(tmp_path, hip_lib, lds_poison, precision):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _ = ao.make_case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version="3.0")
    batch = 9
    x = nn_cases.synthetic_planes(batch, 52, 77).numpy().reshape(-1)
    net = HipAPI(0, batch, d, precision)
    outs = []
    for pattern in (0x00000000, 0x00000000, 0xffffffff, 0x7f7f7f7f, 0x7bff7bff, 0x7f800000):
        assert lds_poison.poison_lds(pattern, pattern, 0, 0) == 0
        v = np.zeros(batch, np.float32)
        p = np.zeros(batch * cfg.nb_policy, np.float32)
        net.predict(x, v, p)
        outs.append((v, p))
    net.close()
    assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all()
    for v, p in outs[1:]:
        assert np.array_equal(v, outs[0][0]) and np.array_equal(p, outs[0][1])


def test_float16p8_runs_as_float16x3_on_the_layer_path(tmp_path, hip_lib):
    """a 192-channel net has no float16p8 kernel on its path: the same launches, the same bits as float16x3"""
    cfg, sd, x = ao.make_case("alphavile-tiny")
    a = run(tmp_path, cfg, sd, x, "float16x3", "alphavile-tiny")
    b = run(tmp_path, cfg, sd, x, "float16p8", "alphavile-tiny")
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)


@pytest.mark.parametrize("precision", ["fp8", "int8"])
def test_fp8_and_int8_are_refused(tmp_path, hip_lib, precision):
    """refused by the builder (the 8-bit GEMMs live in the one-launch tower only); int8 gets a calibration file first, so that what is
    tested is that refusal and not the missing calibration"""
    import glob
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _ = ao.make_case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version="3.0")
    if precision == "int8":
        (path,) = glob.glob(d + "/*.cranet")
        with open(path + ".int8calib", "w") as f:
            f.write(f"crazyara-int8-calibration 1\nboards 1\nblocks {len(cfg.kernels)}\n" + "4 4\n" * len(cfg.kernels))
    with pytest.raises(Exception, match="runs on the one-launch bottleneck tower only"):
        HipAPI(0, 4, d, precision)


def test_op_list_has_one_attention_launch_per_ntb(tmp_path, hip_lib):
    from crazyara_amd.neuralnetapi import HipAPI
    cfg, sd, _ = ao.make_case("alphavile-normal")
    d = nn_cases.export_case(tmp_path, "alphavile-normal", cfg, sd, version="3.0")
    net = HipAPI(0, 4, d, "float16x3")
    names = [n for n, _ in net.time_ops(1)]
    net.close()
    assert names.count("attention") == 2
    assert not {"tower", "tower_x3", "fused_block", "block_x3", "head", "forward", "stem"} & set(names)


def test_root_priors_and_value_match_the_restatement(tmp_path, hip_lib):
    """SearchPool on AlphaVile-tiny, float32, chess positions: the root's priors are the restatement's probabilities of the legal moves,
    the children are sorted by them, and the root's value is the restatement's.  One simulation leaves the root with two values, its own
    evaluation and the backed-up one of the child it expanded: root_value = (v + q) / 2, q = that child's Q from the root's side."""
    from crazyara_amd import env, openings, search
    from crazyara_amd.neuralnetapi import HipAPI
    from oracle import chess_oracle as co
    cfg, sd, _ = ao.make_case("alphavile-tiny")
    d = nn_cases.export_case(tmp_path, "alphavile-tiny", cfg, sd, version="3.0")
    # (a root with a single legal move is not evaluated by the search: it has nothing to choose)
    fens = [f for f in openings.position_fens("chess")[::17] if len(co.Board(f, False, "chess").legal_moves()) > 1][:8]
    net = HipAPI(0, 8, d, "float32")
    st = search.default_settings(mode=1, version_major=3, node_policy_temperature=1.0)
    pool = search.SearchPool(st, net_a=net)
    for f in fens:
        pool.add_position(f, False, "chess")
    stats = pool.run(simulations=1, threads=2)
    assert stats.nn_evals >= len(fens)
    pm = co.PolicyMap(co.MODE_CHESS)
    for i, f in enumerate(fens):
        b = co.Board(f, False, "chess")
        x = torch.from_numpy(co.board_to_planes(b, co.MODE_CHESS, 3, True)[None])
        v, p, _ = ao.predict(cfg, sd, x)
        exp = {b.move_uci(m): float(p[0, pm.index(b, m, True)]) for m in b.legal_moves()}
        moves, visits, q, pri = pool.root_children(i)
        assert len(moves) > 0
        pos = env.Position(f, False, "chess")
        for m, pr in zip(moves, pri):
            assert abs(exp[pos.move_uci(m)] - float(pr)) < 1e-6
        best = max(exp, key=exp.get)                    # children sorted by descending prior: the first is the restatement's argmax
        assert abs(exp[pos.move_uci(moves[0])] - exp[best]) < 1e-7
        info = pool.tree_info(i)
        assert info["root_visits"] == 1 and visits[0] == 1
        assert abs(2.0 * info["root_value"] - float(q[0]) - float(v[0])) < 1e-4
    pool.close()
    net.close()
