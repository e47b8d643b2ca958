"""The index maps of tower_x3_quad_kernel (x3_quad.h, constexpr and host-callable) without a GPU: scripts/studies/x3_quad_maps.cpp prints
what the store side (EXPAND lanes) and the read side (PROJECT lanes, ds_read_b64_tr_b16) compute, and this test plays the hardware's part.

  * The square <-> tile row map is a permutation, and an EXPAND lane's accumulator [t][lg][r] is rank 4 (lg >> 1) + t, file 4 (lg & 1) + r
    at tile row t * 16 + 4 lg + r: a lane owns a 4 x 4 quadrant.
  * The stores of a chunk fill t2T exactly once (a permutation of its 8192 halves), 8-byte aligned.
  * The transposed read, modelled as the ISA describes it (per 16-lane group, lane 4 q + p names row q, columns 4 p ... 4 p + 3; lane i
    receives column i, row q in element q), hands PROJECT lane (l15, lg) the eight channels s2 * 32 + lg * 8 + e of tile row t * 16 + l15 --
    the k of today's fragments -- from where the store side put them.  Every lane's address is in bounds and 8-byte aligned.
  * Banks: no conflict in a ds_write_b64 (16-lane groups, bank (a / 4) % 32) nor in a transposed read (32-lane halves, (a / 4) % 64)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = 128 * 64


def _maps(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "x3_quad_maps")
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "crazyara_amd", "csrc", "nn"),
                    os.path.join(ROOT, "scripts", "studies", "x3_quad_maps.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    rows, lanes, store, read = {}, {}, {}, {}
    for line in out.splitlines():
        kind, *v = line.split()
        v = [int(i) for i in v]
        if kind == "row":
            rows[v[0]] = (v[1], v[2])
        elif kind == "lane":
            lanes[tuple(v[:3])] = v[3]
        elif kind == "store":
            store[tuple(v[:4])] = v[4]
        else:
            read[tuple(v[:5])] = v[5]
    return rows, lanes, store, read


def test_row_map_store_side_and_transposed_read_side_agree(tmp_path):
    rows, lanes, store, read = _maps(tmp_path)
    # the row map
    assert sorted(r for r, _ in rows.values()) == list(range(64))
    assert all(back == sq for sq, (_, back) in rows.items())
    for (t, lg, r), sq in lanes.items():
        assert sq == (4 * (lg >> 1) + t) * 8 + 4 * (lg & 1) + r
        assert rows[sq][0] == t * 16 + 4 * lg + r
    for lg in range(4):                                         # a lane group's 16 accumulators: one quadrant
        assert {lanes[t, lg, r] for t in range(4) for r in range(4)} == {(4 * (lg >> 1) + y) * 8 + 4 * (lg & 1) + x for y in range(4) for x in range(4)}
    # store side: where (channel, tile row) lies
    where = {}
    for (tile, l15, lg, t), off in store.items():
        assert off % 4 == 0 and 0 <= off <= HALVES - 4          # ds_write_b64: 8-byte aligned, in bounds
        for r in range(4):
            key = (tile * 16 + l15, t * 16 + 4 * lg + r)
            assert key not in where
            where[key] = off + r
    assert sorted(where.values()) == list(range(HALVES))
    # read side: the hardware's gather
    for s2 in range(4):
        for hh in range(2):
            for t in range(4):
                for lg in range(4):
                    addr = [read[s2, hh, t, i, lg] for i in range(16)]
                    assert all(a % 4 == 0 and 0 <= a <= HALVES - 4 for a in addr)
                    for i in range(16):
                        for q in range(4):
                            got = addr[4 * q + (i >> 2)] + (i & 3)              # element q of lane i
                            assert got == where[s2 * 32 + lg * 8 + hh * 4 + q, t * 16 + i], (s2, hh, t, lg, i, q)
    # banks (offsets in halves -> bytes; both buffers start 128-byte aligned in the tile region)
    for tile in range(8):
        for t in range(4):
            for lg in range(4):                                 # one ds_write_b64 group: the 16 lanes of a lane group
                banks = [(2 * store[tile, l15, lg, t] // 4 + d) % 32 for l15 in range(16) for d in range(2)]
                assert len(set(banks)) == 32
    for s2 in range(4):
        for hh in range(2):
            for t in range(4):
                for half in range(2):                           # one 32-lane half of a transposed read
                    banks = [(2 * read[s2, hh, t, l15, lg] // 4 + d) % 64 for lg in (2 * half, 2 * half + 1) for l15 in range(16) for d in range(2)]
                    assert len(set(banks)) == 64
