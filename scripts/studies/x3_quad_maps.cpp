// Prints the index maps of tower_x3_quad_kernel (crazyara_amd/csrc/nn/x3_quad.h) as the kernel's two sides compute them, for
// tests/test_x3_quad_maps.py: plain C++, no GPU.
//   c++ -std=c++17 -Icrazyara_amd/csrc/nn scripts/studies/x3_quad_maps.cpp -o x3_quad_maps
// Lines:
//   row <square> <tile row>                          x3q_row, and x3q_square back
//   lane <t> <lg> <r> <square>                       the square of an EXPAND lane's accumulator
//   store <tile> <l15> <lg> <t> <offset in halves>   the half4 an EXPAND lane stores (rows t * 16 + 4 lg ... + 3 of channel tile * 16 + l15)
//   read <s2> <hh> <t> <l15> <lg> <offset>           the address a PROJECT lane supplies to the transposed read
#include <cstdio>

#include "x3_quad.h"

int main() {
    using namespace cra;
    static_assert(x3q_square(x3q_row(37)) == 37 && x3q_row(x3q_lane_square(2, 3, 1)) == 2 * 16 + 4 * 3 + 1, "the maps at compile time");
    for (int sq = 0; sq < 64; ++sq) printf("row %d %d %d\n", sq, x3q_row(sq), x3q_square(x3q_row(sq)));
    for (int t = 0; t < 4; ++t)
        for (int lg = 0; lg < 4; ++lg)
            for (int r = 0; r < 4; ++r) printf("lane %d %d %d %d\n", t, lg, r, x3q_lane_square(t, lg, r));
    for (int tile = 0; tile < 8; ++tile)
        for (int l15 = 0; l15 < 16; ++l15)
            for (int lg = 0; lg < 4; ++lg)
                for (int t = 0; t < 4; ++t) printf("store %d %d %d %d %d\n", tile, l15, lg, t, x3q_store_offset(tile, l15, lg, t));
    for (int s2 = 0; s2 < 4; ++s2)
        for (int hh = 0; hh < 2; ++hh)
            for (int t = 0; t < 4; ++t)
                for (int l15 = 0; l15 < 16; ++l15)
                    for (int lg = 0; lg < 4; ++lg) printf("read %d %d %d %d %d %d\n", s2, hh, t, l15, lg, x3q_read_offset(s2, hh, t, l15, lg));
    return 0;
}
