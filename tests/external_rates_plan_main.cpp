// Stand-alone driver of tps_amd/csrc/plasma_params_host.hpp::split_chemistry (tests/test_external_rates_plan.py builds it with
// plain g++, once without and once with -fsanitize=address,undefined, and runs it as a child process): the chemistry of a
// mixture in two blocks, the reactions with a closed form for the sweeps and the reactions with an external rate coefficient
// (TPSRHS_GRIDFUNCTION_RXN) for the pass of their own.  It walks a list of chemistries and prints, per case, the two blocks --
// per reaction its model, the first rate parameter, the energy, the detailed-balance flag, the first keq parameter,
// table_share, the number of points of its table and the stoichiometry -- or the class of the refusal.  The expected lines are
// written out in Python.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "plasma_params_host.hpp"

namespace {

using namespace tpsrhs;

constexpr int NSP = 3;
const double kGridA[4] = {300.0, 1000.0, 5000.0, 20000.0}, kGridB[4] = {300.0, 1000.0, 5000.0, 20001.0};
const double kValues[4] = {1.0, 2.0, 4.0, 8.0};

struct Rxn {
  int model;
  double p0;      // first rate parameter: A of a closed form, the component of a grid-function reaction
  double energy;  // tells the reactions apart in the output
  int balance;
  const double *grid;  // tabulated: the abscissae
  int reactant[NSP], product[NSP];
};

tpsrhs_chemistry chemistry(const std::vector<Rxn> &rx) {
  tpsrhs_chemistry ch;
  std::memset(&ch, 0, sizeof ch);
  ch.num_reactions = static_cast<int>(rx.size());
  ch.electron_index = 1;
  ch.minimum_temperature = 2000.0;
  for (int r = 0; r < ch.num_reactions; r++) {
    ch.reaction_models[r] = rx[r].model;
    ch.reaction_energies[r] = rx[r].energy;
    ch.detailed_balance[r] = rx[r].balance;
    ch.rate_params[0 + r * TPSRHS_MAXCHEMPARAMS] = rx[r].p0;
    ch.rate_params[1 + r * TPSRHS_MAXCHEMPARAMS] = 1.5;
    ch.rate_params[2 + r * TPSRHS_MAXCHEMPARAMS] = 1.0e6;
    ch.equilibrium_constant_params[0 + r * TPSRHS_MAXCHEMPARAMS] = 10.0 + r;
    for (int sp = 0; sp < NSP; sp++) {
      ch.reactant_stoich[sp + r * NSP] = static_cast<int16_t>(rx[r].reactant[sp]);
      ch.product_stoich[sp + r * NSP] = static_cast<int16_t>(rx[r].product[sp]);
    }
    if (rx[r].model == TPSRHS_TABULATED_RXN) {
      ch.rate_tables[r].n_data = 4;
      ch.rate_tables[r].x_data = rx[r].grid;
      ch.rate_tables[r].f_data = kValues;
    }
  }
  return ch;
}

void print_block(const char *name, const ChemDev &c) {
  std::printf("  %s: reactions %d electron %d min_temperature %g\n", name, c.num_reactions, c.electron_index, c.min_temperature);
  for (int r = 0; r < c.num_reactions; r++) {
    std::printf("    %d: model %d p0 %g p1 %g energy %g balance %d keq0 %g share %d table_n %d stoich", r, c.model[r],
                c.rate[0 + r * TPSRHS_MAXCHEMPARAMS], c.rate[1 + r * TPSRHS_MAXCHEMPARAMS], c.energy[r], c.detailed_balance[r],
                c.keq[0 + r * TPSRHS_MAXCHEMPARAMS], c.table_share[r], c.table[r].n);
    for (int sp = 0; sp < NSP; sp++) std::printf(" %d>%d", c.reactant[sp + r * NSP], c.product[sp + r * NSP]);
    std::printf("\n");
  }
}

void run(const char *name, const std::vector<Rxn> &rx) {
  const tpsrhs_chemistry ch = chemistry(rx);
  ChemDev sweep, ext;
  std::vector<std::vector<double>> homes;  // the coefficients of the placed tables
  int placed = 0;
  std::printf("%s:\n", name);
  try {
    split_chemistry<NSP>(ch, sweep, ext, [&](const tpsrhs_table &t) {
      homes.emplace_back();
      TableDev td = table_coeffs(t, homes.back());
      td.x = homes.back().data();
      td.a = td.x + td.n;
      td.b = td.a + td.n;
      placed++;
      return td;
    });
    print_block("sweep", sweep);
    print_block("external", ext);
    std::printf("  components_needed %d tables_placed %d\n", external_components_needed(ext), placed);
  } catch (const UnsupportedConfig &e) {
    std::printf("  unsupported %s\n", e.what());
  } catch (const std::invalid_argument &e) {
    std::printf("  invalid %s\n", e.what());
  }
}

}  // namespace

int main() {
  const int A = TPSRHS_ARRHENIUS, T = TPSRHS_TABULATED_RXN, G = TPSRHS_GRIDFUNCTION_RXN;
  const Rxn ion = {A, 74072.0, 1.0, 0, nullptr, {0, 1, 1}, {1, 2, 0}}, rec = {A, 34126.0, 2.0, 0, nullptr, {1, 2, 0}, {0, 1, 1}};
  auto as = [](Rxn r, int model, double p0, const double *grid = nullptr) {
    r.model = model;
    r.p0 = p0;
    r.grid = grid;
    return r;
  };
  auto balanced = [](Rxn r) {
    r.balance = 1;
    return r;
  };
  run("no_external", {ion, rec});
  run("both_external", {as(ion, G, 0.0), as(rec, G, 1.0)});
  run("second_external", {ion, as(rec, G, 1.0)});
  run("first_external_component_5", {as(ion, G, 5.0), rec});
  run("balance_external", {balanced(as(ion, G, 0.0))});
  // reaction 0 leaves: the tables on grid A share the root 0 of the compacted list (1 of the caller's), the one on grid B its own
  run("table_moves", {as(ion, G, 2.0), as(rec, T, 0.0, kGridA), as(ion, T, 0.0, kGridB), as(rec, T, 0.0, kGridA), as(ion, A, 7.0),
                      as(rec, G, 0.0), as(ion, T, 0.0, kGridB)});
  run("hoffert_lien_stays", {as(ion, TPSRHS_HOFFERTLIEN, 0.01), as(rec, G, 3.0)});
  run("fractional_component", {as(ion, G, 0.5), rec});
  run("negative_component", {ion, as(rec, G, -1.0)});
  run("nan_component", {ion, as(rec, G, std::nan(""))});
  run("radiative_decay", {ion, as(rec, TPSRHS_RADIATIVE_DECAY, 0.0)});
  run("unknown_model", {ion, as(rec, 5, 0.0)});
  {
    std::vector<Rxn> many(TPSRHS_MAXREACTIONS, as(ion, G, 1.0));
    for (int r = 0; r < TPSRHS_MAXREACTIONS; r += 2) many[r] = as(rec, T, 0.0, kGridA);
    run("every_slot", many);
  }
  std::printf("EXTERNAL_RATES_PLAN DONE\n");
  return 0;
}
