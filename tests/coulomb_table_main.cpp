// TEST INFRASTRUCTURE (tests/test_coulomb_table.py): the polynomial table of the Coulomb fits (tps_amd/csrc/coulomb_table.hpp)
// filled and evaluated on the host, by the routines the device uses -- the fill from the closure's own literals
// (physics_plasma.hpp through the host shim of tests/host_physics), the evaluation FMA by FMA as the kernels run it.  A
// program of its own, so that AddressSanitizer / UndefinedBehaviorSanitizer run it directly.
//   coulomb_table_main info          -> "X0 H NI DEG NFIT" and the eight (c0 c1 c2 c3), hexadecimal floats
//   coulomb_table_main < arguments   -> per argument (one hexadecimal float per line): "1 g0 .. g7" on the table, "0" off it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "physics_plasma.hpp"

int main(int argc, char **argv) {
  using namespace tpsrhs;
  if (argc > 1 && std::strcmp(argv[1], "info") == 0) {
    std::printf("%a %a %d %d %d\n", coulomb::X0, coulomb::H, coulomb::NI, coulomb::DEG, coulomb::NFIT);
    for (int f = 0; f < 8; f++) {
      const double *c = f < 4 ? coll::kFitA[f] : coll::kFitB[f - 4];
      std::printf("%a %a %a %a\n", c[0], c[1], c[2], c[3]);
    }
    return 0;
  }
  std::vector<double> table(coulomb::SIZE);
  coll::coulomb_table_fill(table.data());
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    const double x = std::strtod(line, nullptr);
    if (!coulomb::in_range(x)) {
      std::printf("0\n");
      continue;
    }
    double g[8];
    coulomb::eval<8>(table.data(), x, g);
    std::printf("1");
    for (int f = 0; f < 8; f++) std::printf(" %a", g[f]);
    std::printf("\n");
  }
  return 0;
}
