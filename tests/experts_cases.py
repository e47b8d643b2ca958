"""Shared pieces of the game-phase expert tests: seeded playout positions, expert model directories, pinned call buffers."""
import ctypes as C
import os

import numpy as np

import nn_cases
from crazyara_amd import _capi, env

LICHESS, MOVECOUNT = 0, 1

# case -> (plane layout, build mode of the policy indices, input version of the file name): crazyhouse v1 planes, or chess v3 planes
# with the WDL + plies-to-end heads (four aux outputs per board)
CASE_IO = {"risev2-3": (0, 0, "1.0"), "risev2-19": (0, 0, "1.0"), "risev33-wdlp": (4, 1, "3.0"), "risev33": (4, 1, "3.0")}
POISON = 0x7FC0DEAD


def playout_positions(variant, seed, n_games, max_plies, is960=False, start_index=0, drops=True):
    """Every position of `n_games` seeded random playouts (the start position included), as env.Position clones.  drops=False: a board
    move whenever there is one (uniform crazyhouse playouts keep dropping what they capture and never thin the board out)."""
    lib = _capi.load()
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n_games):
        fen = lib.mi_chess960_start_fen(start_index + 37 * g).decode() if is960 else ""
        pos = env.Position(fen, is960, variant)
        for _ in range(max_plies):
            out.append(pos.clone())
            moves = pos.legal_moves()
            if not moves or pos.terminal() != env.TERMINAL_NONE:
                break
            if not drops:
                board_moves = [m for m in moves if "@" not in pos.move_uci(m)]
                moves = board_moves or moves
            pos.push(moves[int(rng.integers(len(moves)))])
    return out


def positions_by_phase(n_per_phase, seed=7):
    """Chess playout positions sorted into the three lichess phases, at least n_per_phase[p] of phase p (descriptors are variant-neutral:
    a crazyhouse-plane net takes them as it takes any board)."""
    pools = {0: [], 1: [], 2: []}
    s = seed
    while any(len(pools[p]) < n_per_phase[p] for p in range(3)):
        for pos in playout_positions("chess", s, 6, 400):
            pools[pos.game_phase(3, LICHESS)].append(pos)
        s += 1
        assert s < seed + 200, "playouts never reached every phase"
    return pools


def make_batch(pools, counts, seed=0):
    """A shuffled batch with counts[p] positions of lichess phase p."""
    rng = np.random.default_rng(seed)
    batch = []
    for p in range(3):
        batch += pools[p][:counts[p]]
    order = rng.permutation(len(batch))
    return [batch[i] for i in order]


def export_experts(tmpdir, case="risev2-3", seeds=(101, 102, 103), names=("phase0", "phase1", "phase2"), cfgs=None, version=None):
    """A model directory with one subdirectory per expert: the same config, differently seeded weights.  Returns (root, [dir...])."""
    from oracle import rise_oracle as ro
    version = version or CASE_IO.get(case, (0, 0, "1.0"))[2]
    root = os.path.join(str(tmpdir), "experts")
    os.makedirs(root, exist_ok=True)
    dirs = []
    for i, (seed, name) in enumerate(zip(seeds, names)):
        cfg = cfgs[i] if cfgs else nn_cases.CASES[case][0]()
        sd = ro.make_state_dict(cfg, seed=seed, stress=True)
        sub = os.path.join(root, name)
        os.makedirs(sub, exist_ok=True)
        from crazyara_amd import netfile
        netfile.export_rise(os.path.join(sub, f"{cfg.name}-v{version}.cranet"), cfg, sd, input_version=version)
        dirs.append(sub)
    return root, dirs


class CallBuffers:
    """Pinned buffers of one descriptor-fed call: descriptors, gather lists, value, whole vectors, gathered priors, aux (when the nets
    have aux outputs: nb_aux = 4)."""

    def __init__(self, batch, nb_policy, stride=96, layout=0, mode=0, nb_aux=0):
        self.lib = _capi.load()
        self.batch, self.nb_policy, self.stride = batch, nb_policy, stride
        self.layout, self.mode, self.nb_aux = layout, mode, nb_aux
        self._ptrs = []
        self.p_desc, self.descs = self._alloc(batch * 192, np.uint8)
        self.p_idx, self.idx = self._alloc(batch * stride, np.uint16)
        self.p_cnt, self.cnt = self._alloc(batch, np.uint32)
        self.p_value, self.value = self._alloc(batch, np.float32)
        self.p_probs, self.probs = self._alloc(batch * nb_policy, np.float32)
        self.p_gath, self.gathered = self._alloc(batch * stride, np.float32)
        self.p_aux, self.aux = self._alloc(batch * nb_aux, np.float32) if nb_aux else (None, None)

    @classmethod
    def for_net(cls, net, case, stride=96):
        layout, mode, _ = CASE_IO[case]
        return cls(net.get_batch_size(), net.get_nb_policy_values(), stride, layout, mode, net.get_nb_auxiliary_outputs())

    def _alloc(self, n, dtype):
        nbytes = n * np.dtype(dtype).itemsize
        p = self.lib.mi_host_alloc(nbytes)
        assert p, _capi.last_error()
        self._ptrs.append(p)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,)).view(dtype)
        arr[:] = 0
        return p, arr

    def load(self, positions):
        """Descriptors and gather lists (policy indices of the legal moves, at most `stride`) of the positions into slots 0 .. n - 1."""
        self.descs[:] = 0
        self.cnt[:] = 0
        self.idx[:] = 0
        for s, pos in enumerate(positions):
            self.descs[s * 192:(s + 1) * 192] = np.frombuffer(pos.desc(), np.uint8)
            ids = [pos.policy_index(m, self.mode, True) for m in pos.legal_moves()]
            ids = [i for i in ids if 0 <= i < self.nb_policy][:self.stride]
            self.cnt[s] = len(ids)
            self.idx[s * self.stride:s * self.stride + len(ids)] = ids

    def poison(self):
        self.value.view(np.uint32)[:] = POISON
        self.probs.view(np.uint32)[:] = POISON
        self.gathered.view(np.uint32)[:] = POISON
        if self.nb_aux:
            self.aux.view(np.uint32)[:] = POISON

    def submit_boards(self, net, n_valid):
        lib = self.lib
        assert lib.mi_net_submit_boards(net._h, self.p_desc, n_valid, self.layout, self.p_value, self.p_probs, self.p_aux) == 0, _capi.last_error()
        assert lib.mi_net_wait(net._h) == 0, _capi.last_error()

    def submit_gathered(self, net, n_valid):
        lib = self.lib
        assert lib.mi_net_submit_boards_gathered(net._h, self.p_desc, n_valid, self.layout, self.p_idx, self.p_cnt, self.stride, self.p_value,
                                                 self.p_gath, self.p_aux) == 0, _capi.last_error()
        assert lib.mi_net_wait(net._h) == 0, _capi.last_error()

    def close(self):
        for p in self._ptrs:
            self.lib.mi_host_free(p)
        self._ptrs = []
