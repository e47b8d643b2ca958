"""Game-phase expert sets, host side (no GPU): the phase of a board descriptor, discovery of a phase-expert model directory and its
refusals, and the new symbols of the C ABI."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import experts_cases as ec
import nn_cases
from crazyara_amd import _capi, neuralnetapi, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("mi_net_create_experts", "mi_net_num_experts", "mi_net_submit_boards_phases", "mi_net_predict_routed", "mi_expert_dirs",
               "mi_net_set_expert_routing", "mi_desc_game_phase")


@pytest.mark.parametrize("variant,is960,seed,games,plies", [("chess", False, 11, 8, 400), ("crazyhouse", False, 12, 8, 400),
                                                            ("chess", True, 13, 8, 400)])
def test_desc_game_phase_equals_the_positions_phase(hip_lib, variant, is960, seed, games, plies):
    """desc_game_phase over the 192-byte descriptor = mi_pos_game_phase (pinned to Board::get_phase by tests/test_selfplay.py) on every
    position of seeded random playouts, for 1 / 2 / 3 movecount phases and the three lichess phases -- all three of which occur."""
    lib = _capi.load()
    positions = ec.playout_positions(variant, seed, games, plies, is960=is960, drops=variant != "crazyhouse")
    assert len(positions) > 300
    seen = set()
    for pos in positions:
        d = pos.desc()
        for num, definition in ((1, ec.MOVECOUNT), (2, ec.MOVECOUNT), (3, ec.MOVECOUNT), (3, ec.LICHESS)):
            want = pos.game_phase(num, definition)
            got = lib.mi_desc_game_phase(d, num, definition)
            assert got == want, (pos.fen(), num, definition, got, want)
        seen.add(pos.game_phase(3, ec.LICHESS))
    assert seen == {0, 1, 2}, seen


def test_desc_game_phase_refuses_nonsense(hip_lib):
    lib = _capi.load()
    d = ec.playout_positions("chess", 1, 1, 1)[0].desc()
    assert lib.mi_desc_game_phase(None, 3, 0) == -1
    assert lib.mi_desc_game_phase(d, 0, 0) == -1
    assert lib.mi_desc_game_phase(d, 3, 2) == -1


def test_discovery_orders_by_phase_and_skips_phase_none(hip_lib, tmp_path):
    root, dirs = ec.export_experts(tmp_path, names=("model-phase2", "phase0", "x1"))
    os.makedirs(os.path.join(root, "phaseNone"))
    open(os.path.join(root, "README.txt"), "w").write("not a model")
    found = neuralnetapi.expert_dirs(root, 8, ec.LICHESS)
    assert [os.path.basename(d.rstrip("/")) for d in found] == ["phase0", "x1", "model-phase2"]
    assert neuralnetapi.expert_dirs(root + "/", 8, ec.MOVECOUNT) == found


def _refused(root, definition=ec.LICHESS):
    with pytest.raises(ValueError) as e:
        neuralnetapi.expert_dirs(root, 8, definition)
    return str(e.value)


def test_discovery_refusals_name_the_directory(hip_lib, tmp_path):
    cfg, sd, _ = nn_cases.make_case("risev2-3")
    single = nn_cases.export_case(tmp_path, "single", cfg, sd)
    msg = _refused(single)
    assert "single net" in msg and "mi_net_create" in msg and single in msg

    msg = _refused(os.path.join(str(tmp_path), "nowhere"))
    assert "cannot be opened" in msg and "nowhere" in msg

    empty = os.path.join(str(tmp_path), "empty")
    os.makedirs(os.path.join(empty, "phaseNone"))
    msg = _refused(empty)
    assert "no game-phase subdirectory" in msg and empty in msg

    root, _ = ec.export_experts(tmp_path / "twice", names=("phase0", "phase1", "other1"))
    msg = _refused(root)
    assert "phase 1 twice" in msg and "phase1/" in msg and "other1/" in msg

    root, _ = ec.export_experts(tmp_path / "missing", names=("phase0", "phase1", "phase3"))
    msg = _refused(root)
    assert "phase3/ is for game phase 3" in msg and "phase 2 is missing" in msg and root in msg

    root, _ = ec.export_experts(tmp_path / "two", seeds=(1, 2), names=("phase0", "phase1"))
    msg = _refused(root, ec.LICHESS)
    assert "2 expert(s)" in msg and "three phases" in msg and root in msg
    assert len(neuralnetapi.expert_dirs(root, 8, ec.MOVECOUNT)) == 2

    msg = _refused(root, 5)
    assert "game phase definition 5" in msg


def test_experts_must_agree_in_their_design(hip_lib, tmp_path):
    from oracle import rise_oracle as ro
    base = nn_cases.CASES["risev2-3"][0]
    other_in = ro.rise_v2_config(3, 52, 81)
    other_in.name = "risev2-3"
    root, _ = ec.export_experts(tmp_path / "cin", cfgs=[base(), base(), other_in])
    msg = _refused(root)
    assert "disagree in input channels" in msg and "34" in msg and "52" in msg and "phase2/" in msg

    other_pol = ro.rise_v2_config(3, 34, 76)
    other_pol.name = "risev2-3"
    root, _ = ec.export_experts(tmp_path / "pol", cfgs=[base(), other_pol, base()])
    msg = _refused(root)
    assert "disagree in policy size" in msg and str(81 * 64) in msg and str(76 * 64) in msg

    wdlp, plain_value = ro.rise_v33_config(52, 76, True), ro.rise_v33_config(52, 76, False)
    wdlp.name = plain_value.name = "risev33"
    root, _ = ec.export_experts(tmp_path / "aux", cfgs=[wdlp, wdlp, plain_value], version="3.0")
    msg = _refused(root)
    assert "disagree in aux outputs" in msg and "phase0/ has 4" in msg and "phase2/ has 0" in msg and root in msg

    root, dirs = ec.export_experts(tmp_path / "ver")
    f = [x for x in os.listdir(dirs[1]) if x.endswith(".cranet")][0]
    os.rename(os.path.join(dirs[1], f), os.path.join(dirs[1], f.replace("-v1.0", "-v2.0")))
    msg = _refused(root)
    assert "disagree in version" in msg


def test_create_refuses_before_it_touches_a_device(hip_lib, tmp_path):
    """mi_net_create_experts: every precision but float16x3 is refused by name, a single-net directory points at mi_net_create -- both
    are host-side refusals, the same with and without a GPU."""
    lib = _capi.load()
    root, _ = ec.export_experts(tmp_path)
    for prec in (b"float16", b"float32", b"float16p8", b"fp8", b"int8", b"float16x3-unfused", b"float16x3-perblock", b"float16x3-1wg",
                 b"float16x3-3k", b"float16x3-8w", b"float16x3-1b", b"float16x3-2b"):
        assert not lib.mi_net_create_experts(root.encode(), 0, 8, prec, ec.LICHESS)
        assert "float16x3" in _capi.last_error() and prec.decode() in _capi.last_error()
    cfg, sd, _ = nn_cases.make_case("risev2-3")
    single = nn_cases.export_case(tmp_path, "single", cfg, sd)
    assert not lib.mi_net_create_experts(single.encode(), 0, 8, b"float16x3", ec.LICHESS)
    assert "mi_net_create" in _capi.last_error()
    assert lib.mi_net_num_experts(None) == 0


def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    header = open(os.path.join(ROOT, "include", "crazyara_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert "expert_routing" in header


def test_header_with_the_expert_entry_points_is_c99_and_the_settings_mirror_matches(hip_lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc
    src = os.path.join(str(tmp_path), "experts_check.c")
    open(src, "w").write(
        '#include <stddef.h>\n#include "crazyara_hip.h"\n'
        "size_t cra_sizeof_settings(void) { return sizeof(mi_search_settings); }\n"
        "size_t cra_offsetof_expert_routing(void) { return offsetof(mi_search_settings, expert_routing); }\n"
        "int cra_default_routing(void) { mi_search_settings s; mi_search_default_settings(&s); return s.expert_routing; }\n"
        "typedef mi_net* (*create_fn)(const char*, int, int, const char*, int);\n"
        "typedef int (*routed_fn)(mi_net*, const float*, const int*, float*, float*, float*);\n"
        "typedef int (*phases_fn)(mi_net*, const void*, int, int*);\n"
        "create_fn cra_create = mi_net_create_experts;\nrouted_fn cra_routed = mi_net_predict_routed;\n"
        "phases_fn cra_phases = mi_net_submit_boards_phases;\n"
        "int cra_uses(void) { return mi_net_num_experts(NULL) + MI_EXPERT_ROUTING_MAJORITY; }\n")
    so = os.path.join(str(tmp_path), "libexpertscheck.so")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", so,
                    _capi.LIB_PATH], check=True)
    chk = C.CDLL(so)
    chk.cra_sizeof_settings.restype = chk.cra_offsetof_expert_routing.restype = C.c_size_t
    assert chk.cra_sizeof_settings() == C.sizeof(search.SearchSettingsC)
    assert chk.cra_offsetof_expert_routing() == search.SearchSettingsC.expert_routing.offset
    assert chk.cra_default_routing() == 0
    assert search.default_settings().expert_routing == 0
