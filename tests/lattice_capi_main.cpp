// Stand-alone driver of the lattice entries of libtpsrhs.so on a machine without a device (tests/test_lattice_capi.py builds
// it with hipcc, host side only, and runs it as a child process).  An operator cannot be created without a device, so the
// program fills in the two members the host-only entry reads (dim, ne) of a default-constructed tpsrhs_operator and uses
// its address as the handle: tpsrhs_lattice_size touches nothing else, and every refused call returns before any device
// work.  One line per call: "size <dim> <ne> <levels> <status> <points_per_element> <npts>" and
// "refused <entry> <case> <status> <1 when tpsrhs_last_error() names the entry>".
#include <cstdio>
#include <cstring>

#include "../tps_amd/csrc/operator.hpp"

static void refused(const char *entry, const char *what, int status) {
  std::printf("refused %s %s %d %d\n", entry, what, status, std::strstr(tpsrhs_last_error(), entry) != nullptr);
}

int main() {
  tpsrhs_operator op;
  op.order = 3;
  const int cases[2][2] = {{2, 6}, {3, 12}};
  for (const auto &c : cases) {
    op.dim = c[0];
    op.ne = c[1];
    for (int levels : {1, 3, 8}) {
      int64_t ppe = -1, npts = -1;
      const int st = tpsrhs_lattice_size(&op, levels, &ppe, &npts);
      std::printf("size %d %d %d %d %lld %lld\n", op.dim, op.ne, levels, st, static_cast<long long>(ppe), static_cast<long long>(npts));
    }
  }
  double buf[8] = {0};
  int64_t a = -7, b = -7;
  refused("tpsrhs_lattice_size", "null_handle", tpsrhs_lattice_size(nullptr, 3, &a, &b));
  refused("tpsrhs_lattice_size", "null_ppe", tpsrhs_lattice_size(&op, 3, nullptr, &b));
  refused("tpsrhs_lattice_size", "null_npts", tpsrhs_lattice_size(&op, 3, &a, nullptr));
  for (int levels : {0, 9, -1}) {
    refused("tpsrhs_lattice_size", "levels", tpsrhs_lattice_size(&op, levels, &a, &b));
    refused("tpsrhs_lattice_coordinates", "levels", tpsrhs_lattice_coordinates(&op, levels, buf));
    refused("tpsrhs_lattice_fields", "levels", tpsrhs_lattice_fields(&op, levels, 1, buf, buf, 0));
  }
  refused("tpsrhs_lattice_coordinates", "null_handle", tpsrhs_lattice_coordinates(nullptr, 3, buf));
  refused("tpsrhs_lattice_coordinates", "null_out", tpsrhs_lattice_coordinates(&op, 3, nullptr));
  refused("tpsrhs_lattice_fields", "null_handle", tpsrhs_lattice_fields(nullptr, 3, 1, buf, buf, 0));
  refused("tpsrhs_lattice_fields", "null_field", tpsrhs_lattice_fields(&op, 3, 1, nullptr, buf, 1));
  refused("tpsrhs_lattice_fields", "null_out", tpsrhs_lattice_fields(&op, 3, 1, buf, nullptr, 0));
  for (int nrows : {0, -3}) refused("tpsrhs_lattice_fields", "nrows", tpsrhs_lattice_fields(&op, 3, nrows, buf, buf, 0));
  std::printf("untouched %d %d\n", a == -7 && b == -7, buf[0] == 0.0 && buf[7] == 0.0);
  return 0;
}
