"""Game-phase expert sets on the GPU (float16x3): every board of a routed call gets, bit for bit, what the expert of its phase returns
when the boards of that phase are submitted to it alone as a plain net of the same batch size and precision.

Experts are three differently seeded nets of one config.  Positions are chess playout positions of all three lichess phases (the
descriptor is variant-neutral; the nets read crazyhouse v1 planes).  Group sizes sit on both sides of 64 boards: a group of at most 64
runs the split-board forward (as a plain net's call of that size does), a larger one the tower on its own number of workgroups.
"""
import numpy as np
import pytest

import experts_cases as ec
import nn_cases
from crazyara_amd import _capi, env, search
from crazyara_amd.neuralnetapi import HipAPI, HipExperts, ROUTE_MAJORITY, ROUTE_PER_BOARD

pytestmark = pytest.mark.gpu

# (case, batch): phase counts of the routed calls -- groups above and below 64 boards, an empty group, one group only, n_valid < batch.
# risev33-wdlp: chess v3 planes, WDL + plies-to-end heads -- every call of it also carries four aux outputs per board.
CALLS = {
    ("risev2-19", 256): [(86, 85, 85), (200, 40, 16), (256, 0, 0), (100, 0, 156), (70, 70, 10), (30, 20, 10), (0, 65, 64)],
    ("risev2-3", 8): [(3, 3, 2), (8, 0, 0), (4, 0, 1), (0, 2, 6)],
    ("risev33-wdlp", 160): [(70, 66, 24), (160, 0, 0), (0, 65, 64), (20, 30, 10)],
    ("risev33-wdlp", 8): [(3, 3, 2), (4, 0, 1)],
}


@pytest.fixture(scope="module")
def pools():
    return ec.positions_by_phase((256, 256, 256))


@pytest.fixture(scope="module", params=list(CALLS), ids=lambda p: "%s-%d" % p)
def nets(request, tmp_path_factory, hip_lib):
    case, batch = request.param
    root, dirs = ec.export_experts(tmp_path_factory.mktemp("experts"), case=case)
    experts = HipExperts(0, batch, root, "float16x3", ec.LICHESS)
    plain = [HipAPI(0, batch, d, "float16x3") for d in dirs]
    assert experts.get_nb_auxiliary_outputs() == (4 if case == "risev33-wdlp" else 0)
    yield case, batch, experts, plain
    experts.close()
    for n in plain:
        n.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Out:
    """What one descriptor-fed call left in its buffers, for the first n boards; the rows behind them must still hold the poison."""

    def __init__(self, buf, n, gathered):
        self.value = buf.value[:n].copy()
        self.aux = buf.aux[:n * 4].reshape(n, 4).copy() if buf.nb_aux else None
        if gathered:
            self.rows = buf.gathered[:n * buf.stride].reshape(n, -1).copy()
            rest = buf.gathered[n * buf.stride:]
        else:
            self.rows = buf.probs[:n * buf.nb_policy].reshape(n, -1).copy()
            rest = buf.probs[n * buf.nb_policy:]
        self.untouched = bool(np.all(bits(rest) == ec.POISON)) and (not buf.nb_aux or bool(np.all(bits(buf.aux[n * 4:]) == ec.POISON)))


def call(net, buf, n, gathered):
    buf.poison()
    (buf.submit_gathered if gathered else buf.submit_boards)(net, n)
    return Out(buf, n, gathered)


def routed_outputs(experts, buf, n):
    whole, gath = call(experts, buf, n, False), call(experts, buf, n, True)
    # an expert set writes the boards of the call and nothing else: values, aux and rows behind n_valid keep the poison
    assert whole.untouched and gath.untouched
    assert np.all(bits(buf.value[n:]) == ec.POISON)
    return whole, gath


def assert_rows_equal(buf, got, boards, want, what):
    """got (a routed call, indexed by board) against want (the reference call, indexed by position in `boards`)."""
    k = np.arange(len(boards))
    assert np.array_equal(bits(got.value[boards]), bits(want.value[k])), what
    if buf.nb_aux:
        assert np.isfinite(got.aux[boards]).all(), what
        assert np.array_equal(bits(got.aux[boards]), bits(want.aux[k])), what


def test_every_board_gets_its_own_experts_bits(nets, pools):
    """value, whole probabilities, gathered priors and (risev33-wdlp) aux of board b == expert phase(b)'s plain net on its group alone."""
    case, batch, experts, plain = nets
    assert experts.get_num_phases() == 3 and experts.get_batch_size() == batch
    npol = experts.get_nb_policy_values()
    buf, ref = ec.CallBuffers.for_net(experts, case), ec.CallBuffers.for_net(experts, case)
    for c_no, counts in enumerate(CALLS[(case, batch)]):
        positions = ec.make_batch(pools, counts, seed=c_no)
        n = len(positions)
        phases = [p.game_phase(3, ec.LICHESS) for p in positions]
        assert [phases.count(p) for p in range(3)] == list(counts)
        buf.load(positions)
        assert list(experts.route_phases(buf.p_desc, n)) == phases
        whole, gath = routed_outputs(experts, buf, n)
        assert np.isfinite(whole.value).all() and np.isfinite(whole.rows).all()
        if buf.nb_aux:
            assert len({whole.aux[b].tobytes() for b in range(n)}) > n // 2          # (aux differs from board to board: a swapped slot would show)
        for e in range(3):
            boards = [b for b in range(n) if phases[b] == e]
            if not boards:
                continue
            ref.load([positions[b] for b in boards])
            want = call(plain[e], ref, len(boards), False)
            assert_rows_equal(buf, whole, boards, want, (counts, e, "whole"))
            assert np.array_equal(bits(whole.rows[boards]), bits(want.rows)), (counts, e)
            want = call(plain[e], ref, len(boards), True)
            assert_rows_equal(buf, gath, boards, want, (counts, e, "gathered"))
            for k, b in enumerate(boards):
                c = int(buf.cnt[b])
                assert c == int(ref.cnt[k])
                assert np.array_equal(bits(gath.rows[b, :c]), bits(want.rows[k, :c])), (counts, e, b)
                assert np.all(bits(gath.rows[b, c:]) == ec.POISON)          # nothing written beyond a board's own list
    buf.close()
    ref.close()


def test_majority_routing_is_the_majority_experts_plain_net(nets, pools):
    case, batch, experts, plain = nets
    buf, ref = ec.CallBuffers.for_net(experts, case), ec.CallBuffers.for_net(experts, case)
    half = batch // 2
    # (ties go to the lowest phase among the largest counts: std::max_element over the std::map of the phases that occur)
    for counts, winner in (((batch // 4, batch // 2, batch // 4), 1), ((0, half, half), 1), ((half - 1, 1, half), 2)):
        positions = ec.make_batch(pools, counts, seed=9)
        n = len(positions)
        boards = list(range(n))
        buf.load(positions)
        ref.load(positions)
        experts.set_routing(ROUTE_MAJORITY)
        assert list(experts.route_phases(buf.p_desc, n)) == [winner] * n
        whole, gath = routed_outputs(experts, buf, n)
        experts.set_routing(ROUTE_PER_BOARD)
        want = call(plain[winner], ref, n, False)
        assert_rows_equal(buf, whole, boards, want, (counts, "whole"))
        assert np.array_equal(bits(whole.rows), bits(want.rows))
        want = call(plain[winner], ref, n, True)
        assert_rows_equal(buf, gath, boards, want, (counts, "gathered"))
        for b in range(n):
            c = int(buf.cnt[b])
            assert np.array_equal(bits(gath.rows[b, :c]), bits(want.rows[b, :c]))
    buf.close()
    ref.close()


def test_predict_routed_equals_the_descriptor_route_and_predict_is_refused(nets, pools):
    case, batch, experts, plain = nets
    npol = experts.get_nb_policy_values()
    buf = ec.CallBuffers.for_net(experts, case)
    counts = (batch - 2 * (batch // 3), batch // 3, batch // 3)
    positions = ec.make_batch(pools, counts, seed=4)
    buf.load(positions)
    phases = experts.route_phases(buf.p_desc, batch)
    whole, _ = routed_outputs(experts, buf, batch)
    planes = env.planes_from_descs_host(buf.descs.tobytes(), batch, buf.layout, True)
    v2, p2 = np.full(batch, np.nan, np.float32), np.full(batch * npol, np.nan, np.float32)
    a2 = np.full(batch * 4, np.nan, np.float32) if buf.nb_aux else None
    experts.predict_routed(planes, phases, v2, p2, a2)
    assert np.array_equal(bits(whole.value), bits(v2)) and np.array_equal(bits(whole.rows.reshape(-1)), bits(p2))
    if buf.nb_aux:
        assert np.array_equal(bits(whole.aux.reshape(-1)), bits(a2))
    with pytest.raises(RuntimeError, match="mi_net_predict_routed"):
        experts.predict(planes, v2, p2)
    with pytest.raises(RuntimeError, match="game phase 3"):
        experts.predict_routed(planes, np.full(batch, 3), v2, p2)
    with pytest.raises(RuntimeError, match="no launches of its own"):
        experts.time_ops(1)
    with pytest.raises(RuntimeError, match="no launches of its own"):
        experts.forward_device()
    buf.close()


def test_kept_logits_of_a_routed_call_are_the_experts_logits(nets, pools):
    """mi_net_keep_logits on a set: board b's row of the set's d_logits == its expert's plain net's row, where the plain net has one (a
    plain net made for more than 64 boards keeps no logits for a call of at most 64: that call runs on its companion net)."""
    import torch
    case, batch, experts, plain = nets
    lib = _capi.load()
    buf, ref = ec.CallBuffers.for_net(experts, case), ec.CallBuffers.for_net(experts, case)
    counts = CALLS[(case, batch)][0]
    positions = ec.make_batch(pools, counts, seed=0)
    n = len(positions)
    phases = [p.game_phase(3, ec.LICHESS) for p in positions]
    buf.load(positions)
    for net in [experts] + plain:
        assert lib.mi_net_keep_logits(net._h, 1) == 0
    whole = call(experts, buf, n, False)
    logits = torch.as_tensor(experts.device_buffers()["logits"], device="cuda").cpu().numpy()
    checked = 0
    for e in range(3):
        boards = [b for b in range(n) if phases[b] == e]
        if not boards or (batch > 64 and len(boards) <= 64):
            continue
        ref.load([positions[b] for b in boards])
        want = call(plain[e], ref, len(boards), False)
        assert np.array_equal(bits(whole.rows[boards]), bits(want.rows))
        want_logits = torch.as_tensor(plain[e].device_buffers()["logits"], device="cuda").cpu().numpy()[:len(boards)]
        assert np.array_equal(bits(logits[boards]), bits(want_logits)), e
        checked += len(boards)
    assert checked > 0
    # every board's logits are the ones its probabilities came from (also the groups the companion nets ran)
    sm = torch.softmax(torch.from_numpy(logits[:n].astype(np.float64)), 1).numpy()
    assert np.abs(sm - whole.rows).max() < 1e-6
    for net in [experts] + plain:
        assert lib.mi_net_keep_logits(net._h, 0) == 0
    buf.close()
    ref.close()


def test_routed_forward_is_the_same_whatever_the_cus_held_before(nets, pools, lds_poison):
    case, batch, experts, plain = nets
    buf = ec.CallBuffers.for_net(experts, case)
    counts = (batch - 2 * (batch // 3), batch // 3, batch // 3) if batch < 64 else (batch - 96 - 40, 96, 40)
    positions = ec.make_batch(pools, counts, seed=2)
    buf.load(positions)
    outs = []
    for pattern in (0x00000000, 0xffffffff, 0x7f7f7f7f, 0x7bff7bff, 0x7f800000, 0x00000000):
        assert lds_poison.poison_lds(pattern, pattern, 0, 0) == 0
        outs.append(routed_outputs(experts, buf, len(positions)))
    for o in outs[1:]:
        for got, want in zip(o, outs[0]):
            assert np.array_equal(bits(got.value), bits(want.value)) and np.array_equal(bits(got.rows), bits(want.rows))
            if buf.nb_aux:
                assert np.array_equal(bits(got.aux), bits(want.aux))
    buf.close()


@pytest.fixture(scope="module")
def same_weights(tmp_path_factory, hip_lib):
    """Three copies of ONE net as experts, and that net alone."""
    made = {}

    def make(case, batch):
        if (case, batch) not in made:
            seed = 77
            root, dirs = ec.export_experts(tmp_path_factory.mktemp("same"), case=case, seeds=(seed, seed, seed))
            made[(case, batch)] = (HipExperts(0, batch, root, "float16x3", ec.LICHESS), HipAPI(0, batch, dirs[0], "float16x3"))
        return made[(case, batch)]
    yield make
    for a, b in made.values():
        a.close()
        b.close()


@pytest.mark.parametrize("case,batch,counts", [("risev2-19", 256, (86, 85, 85)), ("risev2-19", 256, (65, 70, 66)), ("risev2-3", 8, (3, 3, 2)),
                                               ("risev2-3", 8, (1, 2, 2)), ("risev33-wdlp", 8, (3, 2, 3))])
def test_three_copies_of_one_net_give_the_plain_nets_bits(same_weights, pools, case, batch, counts):
    """Condition: every group has more than 64 boards (tower against tower), or the whole call has at most 25 boards: the split-board
    forward spreads a board over min(10, CUs / boards) workgroups, the same 10 for any group of a call that small.  Between the two the
    split-board forward and the tower differ by design by up to 2e-5."""
    experts, plain = same_weights(case, batch)
    buf, ref = ec.CallBuffers.for_net(experts, case), ec.CallBuffers.for_net(experts, case)
    positions = ec.make_batch(pools, counts, seed=6)
    n = len(positions)
    boards = list(range(n))
    buf.load(positions)
    ref.load(positions)
    whole, gath = routed_outputs(experts, buf, n)
    want = call(plain, ref, n, False)
    assert_rows_equal(buf, whole, boards, want, "whole")
    assert np.array_equal(bits(whole.rows), bits(want.rows))
    want = call(plain, ref, n, True)
    assert_rows_equal(buf, gath, boards, want, "gathered")
    for b in range(n):
        c = int(buf.cnt[b])
        assert np.array_equal(bits(gath.rows[b, :c]), bits(want.rows[b, :c]))
    buf.close()
    ref.close()


def crazyhouse_fens_of_all_phases(n):
    positions = [p for p in ec.playout_positions("crazyhouse", 12, 8, 400, drops=False) if p.terminal() == env.TERMINAL_NONE and p.legal_moves()]
    by = {ph: [p for p in positions if p.game_phase(3, ec.LICHESS) == ph] for ph in range(3)}
    assert all(by.values())
    out = []
    for i in range(n):
        group = by[i % 3]
        out.append(group[(7 * i) % len(group)].fen())
    return out


def test_two_lane_search_on_expert_sets_reproduces_20_times(tmp_path, hip_lib, monkeypatch):
    """The shape of tests/test_lane_determinism_gpu.py on two expert sets: 9 crazyhouse trees of all three phases, two lanes, 4 host
    threads; every batch is recorded and replayed alone on the device."""
    monkeypatch.setenv("CRA_LANE_RECORD", "1")
    root, _ = ec.export_experts(tmp_path)
    fens = crazyhouse_fens_of_all_phases(9)
    sets = [HipExperts(0, 64, root, "float16x3", ec.LICHESS) for _ in range(2)]
    first, differing_runs, replay_words, reports = None, [], 0, []
    for run in range(20):
        st = search.default_settings(mode=0, version_major=1, batch_size=16, seed=3)
        pool = search.SearchPool(st, net_a=sets[0], net_b=sets[1])
        for f in fens:
            pool.add_position(f, False, "crazyhouse")
        pool.run(simulations=240, threads=4)
        dumps = [pool.tree_dump(i).tobytes() for i in range(len(fens))]
        bad, text = pool.debug_replay()
        replay_words += bad
        if bad and len(reports) < 3:
            reports.append(text[-800:])
        pool.close()
        if first is None:
            first = dumps
        elif dumps != first:
            differing_runs.append(run)
    for s in sets:
        s.close()
    assert replay_words == 0, reports
    assert not differing_runs, differing_runs


@pytest.mark.parametrize("routing", [ROUTE_PER_BOARD, ROUTE_MAJORITY])
def test_search_on_three_copies_of_one_net_builds_the_plain_nets_tree(same_weights, routing):
    """Batches of at most 8 boards (the condition of test_three_copies_of_one_net_give_the_plain_nets_bits)."""
    experts, plain = same_weights("risev2-3", 8)
    fens = crazyhouse_fens_of_all_phases(2)
    dumps = []
    for net in (experts, plain):
        st = search.default_settings(mode=0, version_major=1, batch_size=4, seed=5, expert_routing=routing)
        pool = search.SearchPool(st, net_a=net)
        for f in fens:
            pool.add_position(f, False, "crazyhouse")
        pool.run(simulations=200, threads=1)
        dumps.append([pool.tree_dump(i).tobytes() for i in range(len(fens))])
        pool.close()
    assert dumps[0] == dumps[1]


def test_a_pools_routing_is_handed_over_per_call_and_the_nets_own_stays(tmp_path, hip_lib, monkeypatch):
    """Differently seeded experts: a pool with expert_routing = majority builds other trees than one that routes per board (all three
    phases are among the roots), its recorded batches replay bit for bit, and what mi_net_set_expert_routing set on the net -- the
    routing of direct calls -- is what it was, whichever pool used the set last."""
    monkeypatch.setenv("CRA_LANE_RECORD", "1")
    root, _ = ec.export_experts(tmp_path)
    experts = HipExperts(0, 64, root, "float16x3", ec.LICHESS)
    experts.set_routing(ROUTE_MAJORITY)
    fens = crazyhouse_fens_of_all_phases(6)
    buf = ec.CallBuffers.for_net(experts, "risev2-3")
    buf.load([env.Position(f, False, "crazyhouse") for f in fens])
    dumps = {}
    for routing in (ROUTE_PER_BOARD, ROUTE_MAJORITY, ROUTE_PER_BOARD):
        st = search.default_settings(mode=0, version_major=1, batch_size=8, seed=5, expert_routing=routing)
        pool = search.SearchPool(st, net_a=experts)
        for f in fens:
            pool.add_position(f, False, "crazyhouse")
        pool.run(simulations=120, threads=1)
        d = [pool.tree_dump(i).tobytes() for i in range(len(fens))]
        bad, text = pool.debug_replay()
        pool.close()
        assert bad == 0, text[-800:]
        assert dumps.setdefault(routing, d) == d
        assert len(set(experts.route_phases(buf.p_desc, len(fens)))) == 1          # the net's own routing: still majority
    assert dumps[ROUTE_PER_BOARD] != dumps[ROUTE_MAJORITY]
    buf.close()
    experts.close()
