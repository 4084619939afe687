// Host check of the packed table image (tps_amd/csrc/tab_image.hpp): for one block shape after the other, the image the host
// builds once (make_tab_image) against the LDS copy the lanes of a block make from the same tables (tab_lane_copy, the body
// of kernels.hpp::load_tables), member by member and bit by bit.  A program of its own, built with the sanitizers by
// tests/test_tab_image.py; prints one line per shape, "dim p nc doubles" and the number of differing words per member.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "tab_image.hpp"

using namespace tpsrhs;

template <int N>
static int differing(const double (&a)[N], const double (&b)[N]) {
  int bad = 0;
  for (int i = 0; i < N; i++) bad += std::memcmp(&a[i], &b[i], sizeof(double)) != 0;
  return bad;
}

template <int DIM, int P, int NC>
static int check() {
  typedef Cfg<DIM, P, NC> C;
  const Tables1D src = make_tables(P, DIM, NC, NC);
  // what the lanes of a block leave in LDS: every word starts as a NaN with a payload no table holds
  Tab<C> lanes;
  const uint64_t poison = 0x7ff8dead0000beefull;
  for (size_t i = 0; i < sizeof(lanes) / sizeof(double); i++) std::memcpy(reinterpret_cast<double *>(&lanes) + i, &poison, 8);
  for (int tid = 0; tid < C::BLOCK; tid++) tab_lane_copy<C>(lanes, src, tid);
  const Tab<C> image = make_tab_image<C>(src);
  int iw_bad = 0;
  for (int i = 0; i < C::N1; i++) {
    const double q = 1.0 / src.w[i];
    iw_bad += std::memcmp(&image.iw[i], &q, 8) != 0;
  }
  int untouched = 0;
  for (size_t i = 0; i < sizeof(lanes) / sizeof(double); i++)
    untouched += std::memcmp(reinterpret_cast<const double *>(&lanes) + i, &poison, 8) == 0;
  const int bad[] = {differing(image.x, lanes.x),   differing(image.w, lanes.w),   differing(image.iw, lanes.iw),
                     differing(image.D, lanes.D),   differing(image.b0, lanes.b0), differing(image.b1, lanes.b1),
                     differing(image.xq, lanes.xq), differing(image.wq, lanes.wq), differing(image.B, lanes.B),
                     differing(image.xv, lanes.xv), differing(image.wv, lanes.wv)};
  std::printf("%d %d %d %zu", DIM, P, NC, sizeof(image) / sizeof(double));
  int total = iw_bad + untouched + (std::memcmp(&image, &lanes, sizeof(image)) != 0);
  for (int b : bad) {
    std::printf(" %d", b);
    total += b;
  }
  std::printf(" iw %d untouched %d\n", iw_bad, untouched);
  return total;
}

int main() {
  int bad = 0;
  bad += check<3, 3, 0>();  // the shape of the staged prologue (kernels.hpp::StagedCfg)
  // ... and the other shapes that are built, should the image ever serve them
  bad += check<3, 1, 0>() + check<3, 2, 0>() + check<3, 4, 0>() + check<3, 5, 0>();
  bad += check<2, 1, 0>() + check<2, 2, 0>() + check<2, 3, 0>() + check<2, 4, 0>() + check<2, 5, 0>();
  bad += check<3, 1, 1>() + check<3, 2, 1>() + check<3, 3, 1>() + check<2, 1, 1>() + check<2, 2, 1>() + check<2, 3, 1>();
  return bad ? 1 : 0;
}
