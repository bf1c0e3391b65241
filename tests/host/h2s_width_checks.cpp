// h2s_width_checks.cpp -- what csrc/score_shapes.hpp says of every width the shared-sigma engines take, one line per D = 1 .. 48:
//   D KQF KLF h2p_fits h2c_built h2s_msplit_direct
// tests/test_h2s_width_cases_cpu.py builds it with the host compiler and holds tests/h2s_width_cases.py's expected kernel names
// (computed there from the formulas alone) against it.
#include "score_shapes.hpp"

#include <cstdio>

int main() {
    for (int D = 1; D <= 48; D++) {
        const int kqf = (3 * D + 15) / 16, klf = (3 * D + 2 + 15) / 16;
        std::printf("%d %d %d %d %d %d\n", D, kqf, klf, (int)sr::h2p_fits(kqf, klf), (int)sr::h2c_built(D, klf), (int)sr::h2s_msplit_direct(klf));
    }
    return 0;
}
