// plan_limiter (tps_amd/csrc/limiter.hpp) on the host, through the wrapper every entry point of the C ABI runs its body in
// (status.hpp: guarded): one line per case, `<name>|<status>|<rows resolved>|<covers species>|<message>`, which
// tests/test_limiter_plan.py reads.  No device, no HIP.
#include <cmath>
#include <cstdio>
#include <string>

#include "../tps_amd/csrc/limiter.hpp"
#include "../tps_amd/csrc/status.hpp"

using namespace tpsrhs;

namespace {
LimiterFacts dry_air_2d() {
  LimiterFacts f;
  f.neq = 4, f.nvel = 2, f.sp_first = f.sp_last = 4, f.dry_air = true, f.gamma = 1.4;
  return f;
}
LimiterFacts ternary_2d() {  // ambipolar ternary mixture: one species row
  LimiterFacts f;
  f.neq = 5, f.nvel = 2, f.sp_first = 4, f.sp_last = 5, f.dry_air = false;
  return f;
}
LimiterFacts six_species_2t_2d() {  // five species rows, then the electron energy
  LimiterFacts f;
  f.neq = 10, f.nvel = 2, f.sp_first = 4, f.sp_last = 9, f.dry_air = false;
  return f;
}
LimiterFacts table_gas() {
  LimiterFacts f;
  f.neq = 5, f.nvel = 3, f.sp_first = f.sp_last = 5, f.dry_air = false;
  return f;
}
tpsrhs_limiter lim(int num_rows, std::initializer_list<int> rows, std::initializer_list<double> floors, double pf) {
  tpsrhs_limiter l = {};
  l.num_rows = num_rows;
  int i = 0;
  for (int r : rows) l.rows[i++] = r;
  i = 0;
  for (double f : floors) l.floors[i++] = f;
  l.pressure_floor = pf;
  return l;
}
void run(const char *name, const tpsrhs_limiter &l, const LimiterFacts &f, bool in_loop) {
  LimiterPlan pl;
  const int st = guarded([&] { pl = plan_limiter(l, f, in_loop, in_loop ? "tpsrhs_limiter_configure" : "tpsrhs_limit"); });
  std::string rows;
  for (int i = 0; i < pl.num_rows; i++) rows += (i ? "," : "") + std::to_string(pl.rows[i]);
  std::printf("%s|%d|%s|%d|%s\n", name, st, rows.c_str(), pl.covers_species ? 1 : 0, st ? last_error().c_str() : "");
}
}  // namespace

int main() {
  const double nan = std::nan("");
  run("ok_rows", lim(2, {0, 3}, {0.1, 0.0}, 0.0), dry_air_2d(), false);
  run("ok_pressure", lim(1, {0}, {0.1}, 10.0), dry_air_2d(), true);
  run("default_dry_air_is_empty", lim(-1, {}, {}, 0.0), dry_air_2d(), true);
  run("default_table_gas_is_empty", lim(-1, {}, {}, 0.0), table_gas(), true);
  run("default_ternary", lim(-1, {}, {}, 0.0), ternary_2d(), true);
  run("default_six_species", lim(-1, {}, {}, 0.0), six_species_2t_2d(), true);
  run("row_negative", lim(1, {-1}, {0.0}, 0.0), dry_air_2d(), false);
  run("row_too_large", lim(1, {4}, {0.0}, 0.0), dry_air_2d(), false);
  run("row_twice", lim(2, {1, 1}, {0.0, 0.0}, 0.0), dry_air_2d(), false);
  run("num_rows_below_minus_one", lim(-2, {}, {}, 0.0), dry_air_2d(), false);
  run("num_rows_above_neq", lim(5, {0, 1, 2, 3, 3}, {0, 0, 0, 0, 0}, 0.0), dry_air_2d(), false);
  run("floor_nan", lim(1, {0}, {nan}, 0.0), dry_air_2d(), false);
  run("pressure_floor_negative", lim(1, {0}, {0.1}, -1.0), dry_air_2d(), false);
  run("pressure_floor_nan", lim(1, {0}, {0.1}, nan), dry_air_2d(), false);
  run("pressure_without_row_0", lim(1, {3}, {0.1}, 10.0), dry_air_2d(), false);
  run("pressure_with_row_0_at_floor_0", lim(1, {0}, {0.0}, 10.0), dry_air_2d(), false);
  run("pressure_on_a_mixture", lim(1, {0}, {0.1}, 10.0), ternary_2d(), false);
  run("pressure_on_the_table_gas", lim(1, {0}, {0.1}, 10.0), table_gas(), false);
  run("some_species_rows_in_the_loop", lim(2, {4, 6}, {0.0, 0.0}, 0.0), six_species_2t_2d(), true);
  run("some_species_rows_in_one_application", lim(2, {4, 6}, {0.0, 0.0}, 0.0), six_species_2t_2d(), false);
  run("no_species_row_in_the_loop", lim(1, {0}, {0.1}, 0.0), six_species_2t_2d(), true);
  std::printf("LIMITER PLAN DONE\n");
  return 0;
}
