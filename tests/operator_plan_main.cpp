// Stand-alone driver of tps_amd/csrc/operator_plan.hpp and element_geometry.hpp (tests/test_operator_plan.py builds it with
// plain g++, once without and once with -fsanitize=address,undefined, and runs it as a child process).  It walks a table of
// configurations and prints, per row, the plan's fields or the class of the refusal and its message; then the element sizes
// of two boxes and, for warped elements, the largest entry of M M^-1 - I with a mass matrix it integrates itself.  The
// expected lines are written out in Python.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/tpsrhs.h"
#include "../tps_amd/csrc/element_geometry.hpp"
#include "../tps_amd/csrc/operator_plan.hpp"

namespace {

struct Row {
  std::string name;
  int dim;
  tpsrhs_disc disc;
  tpsrhs_physics phys;
  std::vector<tpsrhs_bc> bcs;
};

const double kT[4] = {300.0, 1000.0, 5000.0, 20000.0}, kE[4] = {2.0e5, 8.0e5, 6.0e6, 9.0e7}, kDown[4] = {2.0e5, 8.0e5, 7.0e5, 9.0e7};

tpsrhs_disc disc(int order, int basis = 0, int rule = 0, int axi = 0, int roe = 0) {
  tpsrhs_disc d;
  std::memset(&d, 0, sizeof d);
  d.order = order;
  d.basis_type = basis;
  d.int_rule_type = rule;
  d.axisymmetric = axi;
  d.use_roe = roe;
  return d;
}
tpsrhs_physics dry(int eq = TPSRHS_NS) {
  tpsrhs_physics p;
  std::memset(&p, 0, sizeof p);
  p.eq_system = eq;
  p.working_fluid = TPSRHS_DRY_AIR;
  return p;
}
tpsrhs_physics mix(int nsp, int ambi, int two_t, int transport) {
  tpsrhs_physics p = dry();
  p.working_fluid = TPSRHS_USER_DEFINED;
  p.mixture.num_species = nsp;
  p.mixture.is_electron_included = 1;
  p.mixture.ambipolar = ambi;
  p.mixture.two_temperature = two_t;
  p.transport_model = transport;
  return p;
}
tpsrhs_physics lte(const double *energy = kE) {
  tpsrhs_physics p = dry();
  p.working_fluid = TPSRHS_LTE_FLUID;
  for (tpsrhs_table *t : {&p.lte.energy_table, &p.lte.gas_constant_table, &p.lte.sound_speed_table, &p.lte.viscosity_table,
                          &p.lte.conductivity_table, &p.lte.electric_conductivity_table}) {
    t->n_data = 4;
    t->x_data = kT;
    t->f_data = energy;
  }
  return p;
}
tpsrhs_bc bc(int attribute, int category, int type, std::vector<double> data = {}) {
  tpsrhs_bc b;
  std::memset(&b, 0, sizeof b);
  b.attribute = attribute;
  b.category = category;
  b.type = type;
  for (size_t k = 0; k < data.size(); k++) b.data[k] = data[k];
  return b;
}
tpsrhs_physics with_sgs(tpsrhs_physics p, int model, double c = 0.0) {
  p.sgs.model_type = model;
  p.sgs.model_const = c;
  return p;
}
tpsrhs_physics with_sponge(tpsrhs_physics p, double n0, double n1, double n2, double width, double ratio) {
  p.visc_sponge.enabled = 1;
  p.visc_sponge.normal[0] = n0;
  p.visc_sponge.normal[1] = n1;
  p.visc_sponge.normal[2] = n2;
  p.visc_sponge.point[0] = 0.25;
  p.visc_sponge.point[1] = -0.5;
  p.visc_sponge.point[2] = 2.0;
  p.visc_sponge.width = width;
  p.visc_sponge.ratio = ratio;
  return p;
}
std::vector<tpsrhs_bc> walls(int n) {
  std::vector<tpsrhs_bc> v;
  for (int i = 0; i < n; i++) v.push_back(bc(i + 1, TPSRHS_WALL, TPSRHS_INV));
  return v;
}

std::vector<Row> table() {
  const int MIN = TPSRHS_ARGON_MINIMAL, MIXT = TPSRHS_ARGON_MIXTURE, CONST = TPSRHS_CONSTANT;
  std::vector<Row> r;
  // the discretisation and the working fluid
  r.push_back({"dry3d_gl", 3, disc(2), dry(), {}});
  r.push_back({"dry2d_gl", 2, disc(5), dry(TPSRHS_EULER), {}});
  r.push_back({"dry3d_gll", 3, disc(3, 1, 1), dry(), {}});
  r.push_back({"dry2d_gll", 2, disc(1, 1, 1), dry(), {}});
  r.push_back({"basis_gl_rule_gll", 3, disc(2, 0, 1), dry(), {}});
  r.push_back({"basis_gll_rule_gl", 3, disc(2, 1, 0), dry(), {}});
  r.push_back({"dry_axi", 2, disc(2, 0, 0, 1), dry(), {}});
  r.push_back({"gll_axi", 2, disc(2, 1, 1, 1), dry(), {}});
  r.push_back({"axi_on_3d_mesh", 3, disc(2, 0, 0, 1), dry(), {}});
  {
    tpsrhs_physics p = dry();
    p.working_fluid = 7;
    r.push_back({"unknown_fluid", 3, disc(2), p, {}});
  }
  r.push_back({"lte_axi", 2, disc(2, 0, 0, 1), lte(), {}});
  r.push_back({"lte_planar", 2, disc(2), lte(), {}});
  r.push_back({"lte_3d", 3, disc(2), lte(), {}});
  r.push_back({"roe_2d", 2, disc(2, 0, 0, 0, 1), dry(), {}});
  r.push_back({"roe_3d", 3, disc(2, 0, 0, 0, 1), dry(), {}});
  r.push_back({"roe_axi", 2, disc(2, 0, 0, 1, 1), dry(), {}});
  r.push_back({"roe_mixture", 2, disc(2, 0, 0, 0, 1), mix(3, 1, 0, MIN), {}});
  r.push_back({"ns_passive", 3, disc(2), dry(TPSRHS_NS_PASSIVE), {}});
  r.push_back({"order_0", 3, disc(0), dry(), {}});
  r.push_back({"order_1", 3, disc(1), dry(), {}});
  r.push_back({"order_5", 3, disc(5), dry(), {}});
  r.push_back({"order_6", 3, disc(6), dry(), {}});
  r.push_back({"order_6_mixture", 3, disc(6), mix(3, 1, 0, MIN), {}});
  // boundary conditions
  r.push_back({"dry_16_bcs", 3, disc(2), dry(), walls(16)});
  r.push_back({"dry_17_bcs", 3, disc(2), dry(), walls(17)});
  r.push_back({"mixture_8_bcs", 3, disc(2), mix(3, 1, 0, MIN), walls(8)});
  r.push_back({"mixture_9_bcs", 3, disc(2), mix(3, 1, 0, MIN), walls(9)});
  r.push_back({"reflecting_set", 3, disc(2), dry(),
               {bc(1, TPSRHS_INLET, TPSRHS_SUB_DENS_VEL, {1.2, 30.0, 0.0, 0.0}), bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P, {101300.0}),
                bc(3, TPSRHS_WALL, TPSRHS_VISC_ISOTH, {300.0}), bc(4, TPSRHS_WALL, TPSRHS_VISC_ADIAB), bc(5, TPSRHS_WALL, TPSRHS_SLIP)}});
  r.push_back({"nr_outlet", 3, disc(2), dry(), {bc(1, TPSRHS_WALL, TPSRHS_INV), bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P_NR, {101300.0})}});
  r.push_back({"nr_inlet_2d", 2, disc(2), dry(), {bc(1, TPSRHS_INLET, TPSRHS_SUB_VEL_CONST_ENT, {1.2, 30.0, 0.0, 0.0})}});
  r.push_back({"nr_outlet_mixture", 3, disc(2), mix(3, 1, 0, MIN), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P_NR, {101300.0})}});
  r.push_back({"nr_outlet_axi", 2, disc(2, 0, 0, 1), dry(), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P_NR, {101300.0})}});
  r.push_back({"nr_outlet_lte", 2, disc(2, 0, 0, 1), lte(), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P_NR, {101300.0})}});
  r.push_back({"massflow_with_area", 3, disc(2), dry(), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_MF_NR, {0.3, 0, 0, 0, 0, 0, 0, 1.5})}});
  r.push_back({"massflow_without_area", 3, disc(2), dry(), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_MF_NR_PW, {0.3})}});
  r.push_back({"face_inlet_3d", 3, disc(2), dry(), {bc(1, TPSRHS_INLET, TPSRHS_SUB_DENS_VEL_FACE_Y, {1.2, 30.0, 0.0, 0.0})}});
  r.push_back({"face_inlet_2d", 2, disc(2), dry(), {bc(1, TPSRHS_INLET, TPSRHS_SUB_DENS_VEL_FACE_X, {1.2, 30.0, 0.0, 0.0})}});
  r.push_back({"uniform_inlet", 3, disc(2), dry(), {bc(1, TPSRHS_WALL, TPSRHS_INV), bc(5, TPSRHS_INLET, TPSRHS_UNI_DENS_VEL)}});
  r.push_back({"general_wall_dry_air", 3, disc(2), dry(), {bc(3, TPSRHS_WALL, TPSRHS_VISC_GNRL, {300.0, 300.0, TPSRHS_ISOTH, TPSRHS_ISOTH})}});
  // viscous_general walls of a mixture: every (two_temperature, ambipolar, heavy condition, electron condition)
  for (int two_t = 0; two_t < 2; two_t++)
    for (int ambi = 0; ambi < 2; ambi++)
      for (int hc = TPSRHS_ADIAB; hc <= TPSRHS_NONE_THMCND; hc++)
        for (int ec = TPSRHS_ADIAB; ec <= TPSRHS_NONE_THMCND; ec++)
          r.push_back({"general_wall_t" + std::to_string(two_t) + "_a" + std::to_string(ambi) + "_h" + std::to_string(hc) + "_e" + std::to_string(ec),
                       2, disc(2), mix(3, ambi, two_t, CONST),
                       {bc(3, TPSRHS_WALL, TPSRHS_VISC_GNRL, {300.0, 11000.0, static_cast<double>(hc), static_cast<double>(ec)})}});
  // mixtures: species count, transport, the family unit
  r.push_back({"ternary_3d_p3", 3, disc(3), mix(3, 1, 0, MIN), {}});
  r.push_back({"ternary_3d_p4", 3, disc(4), mix(3, 1, 0, MIN), {}});
  r.push_back({"ternary_3d_gll_p3", 3, disc(3, 1, 1), mix(3, 1, 0, MIN), {}});
  r.push_back({"ternary_2d_not_ambipolar_2t", 2, disc(2), mix(3, 0, 1, CONST), {}});
  r.push_back({"seven_axi_p3", 2, disc(3, 0, 0, 1), mix(7, 1, 1, MIXT), {}});
  r.push_back({"seven_axi_p4", 2, disc(4, 0, 0, 1), mix(7, 1, 1, MIXT), {}});
  r.push_back({"seven_3d_not_ambipolar_p5", 3, disc(5), mix(7, 0, 0, MIXT), {}});
  r.push_back({"eight_constant", 3, disc(2), mix(8, 1, 0, CONST), {}});
  r.push_back({"eight_argon_mixture", 3, disc(2), mix(8, 1, 0, MIXT), {}});
  r.push_back({"four_argon_minimal", 3, disc(2), mix(4, 1, 0, MIN), {}});
  r.push_back({"four_argon_mixture", 2, disc(1), mix(4, 1, 0, MIXT), {}});
  r.push_back({"two_species", 3, disc(2), mix(2, 1, 0, CONST), {}});
  r.push_back({"nine_species", 3, disc(2), mix(9, 1, 0, CONST), {}});
  r.push_back({"lte_transport_for_a_mixture", 3, disc(2), mix(3, 1, 0, TPSRHS_LTE_TRANSPORT), {}});
  {
    tpsrhs_physics p = mix(3, 1, 0, MIN);
    p.mixture.is_electron_included = 0;
    r.push_back({"no_electrons", 3, disc(2), p, {}});
  }
  // sub-grid scale models and the viscous sponge
  r.push_back({"smagorinsky_3d", 3, disc(2), with_sgs(dry(), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"sigma_3d", 3, disc(2), with_sgs(dry(), TPSRHS_SGS_SIGMA), walls(2)});
  r.push_back({"sigma_3d_own_constant", 3, disc(2), with_sgs(dry(), TPSRHS_SGS_SIGMA, 0.2), {}});
  r.push_back({"smagorinsky_2d", 2, disc(2), with_sgs(dry(), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"smagorinsky_gll", 3, disc(2, 1, 1), with_sgs(dry(), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"smagorinsky_nr_outlet", 3, disc(2), with_sgs(dry(), TPSRHS_SGS_SMAGORINSKY), {bc(2, TPSRHS_OUTLET, TPSRHS_SUB_P_NR, {101300.0})}});
  r.push_back({"unknown_sgs_model", 3, disc(2), with_sgs(dry(), 5), {}});
  r.push_back({"smagorinsky_mixture", 2, disc(2), with_sgs(mix(3, 1, 0, MIN), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"smagorinsky_axi", 2, disc(2, 0, 0, 1), with_sgs(dry(), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"smagorinsky_lte", 2, disc(2, 0, 0, 1), with_sgs(lte(), TPSRHS_SGS_SMAGORINSKY), {}});
  r.push_back({"sponge_dry_2d", 2, disc(2), with_sponge(dry(), 3.0, 4.0, 7.0, 0.3, 25.0), {}});
  r.push_back({"sponge_dry_3d_sigma", 3, disc(2), with_sgs(with_sponge(dry(), 1.0, 2.0, 2.0, 1.5, 8.0), TPSRHS_SGS_SIGMA), {}});
  r.push_back({"sponge_dry_zero_width", 3, disc(2), with_sponge(dry(), 1.0, 0.0, 0.0, 0.0, 8.0), {}});
  r.push_back({"sponge_dry_2d_normal_in_z_only", 2, disc(2), with_sponge(dry(), 0.0, 0.0, 1.0, 1.0, 8.0), {}});
  r.push_back({"sponge_mixture_2d", 2, disc(2), with_sponge(mix(3, 1, 0, MIN), 0.0, 3.0, 0.0, 0.2, 11.0), {}});
  r.push_back({"sponge_dry_axi", 2, disc(2, 0, 0, 1), with_sponge(dry(), 4.0, 3.0, 0.0, 0.5, 2.0), {}});
  r.push_back({"sponge_lte", 2, disc(2, 0, 0, 1), with_sponge(lte(), 1.0, 0.0, 0.0, 0.5, 2.0), {}});
  r.push_back({"sponge_mixture_3d", 3, disc(2), with_sponge(mix(3, 1, 0, MIN), 1.0, 0.0, 0.0, 1.0, 2.0), {}});
  r.push_back({"sponge_mixture_2d_negative_width", 2, disc(2), with_sponge(mix(3, 1, 0, MIN), 1.0, 0.0, 0.0, -1.0, 2.0), {}});
  r.push_back({"sponge_mixture_2d_zero_normal", 2, disc(2), with_sponge(mix(3, 1, 0, MIN), 0.0, 0.0, 5.0, 1.0, 2.0), {}});
  // the tables of the table gas
  {
    tpsrhs_physics p = lte();
    p.lte.conductivity_table.f_log_scale = 1;
    r.push_back({"lte_log_scale", 2, disc(2, 0, 0, 1), p, {}});
  }
  r.push_back({"lte_energy_not_increasing", 2, disc(2, 0, 0, 1), lte(kDown), {}});
  return r;
}

void print_plan(const Row &row) {
  using namespace tpsrhs;
  try {
    const OperatorPlan p = plan_operator(row.dim, row.disc, row.phys, static_cast<int>(row.bcs.size()), row.bcs.data());
    std::printf("%s: plan nc %d dim %d order %d nvel %d neq %d sp %d %d plasma %d lte %d heavy2d %d les %d any_nr %d sponge %d "
                "n %.17g %.17g %.17g p %.17g %.17g %.17g width %.17g ratio %.17g sgs_const %.17g transport %d unit %s\n",
                row.name.c_str(), p.nc, p.dim, p.order, p.nvel, p.neq, p.sp_first, p.sp_last, p.plasma, p.lte, p.heavy2d, p.les, p.any_nr, p.sponge,
                p.sponge_n[0], p.sponge_n[1], p.sponge_n[2], p.sponge_p[0], p.sponge_p[1], p.sponge_p[2], p.sponge_width,
                p.sponge_ratio, p.sgs_const, p.transport, p.unit.empty() ? "-" : p.unit.c_str());
  } catch (const Unsupported &e) {
    std::printf("%s: unsupported %s\n", row.name.c_str(), e.what());
  } catch (const std::invalid_argument &e) {
    std::printf("%s: invalid %s\n", row.name.c_str(), e.what());
  }
}

// corners of one element in lexicographic order: the unit cube scaled by `len`, each corner moved by `warp` times a fixed
// pattern (0: an axis-aligned box)
std::vector<double> element(int dim, const double *len, double warp) {
  const int nv = 1 << dim;
  std::vector<double> v(static_cast<size_t>(nv) * dim);
  for (int c = 0; c < nv; c++)
    for (int d = 0; d < dim; d++)
      v[c * dim + d] = len[d] * ((c >> d) & 1) + warp * std::sin(1.0 + 2.3 * c + 0.7 * d);
  return v;
}

// max |M Minv - I| with M_jk = sum_q w_q det J(q) phi_j(q) phi_k(q) integrated here, Minv from the library
double mass_inverse_defect(int dim, int order) {
  using namespace tpsrhs;
  const double len[3] = {0.9, 0.6, 0.75};
  const std::vector<double> V = element(dim, len, 0.07);
  const std::vector<double> Minv = inverse_mass_matrices(V, dim, order, 1);
  const Tables1D t = make_tables(order, dim, 1, 1);
  const int n1 = order + 1, qv = rule_points(1, 2 * order), nv = 1 << dim;
  int npe = 1, nq = 1;
  for (int d = 0; d < dim; d++) npe *= n1, nq *= qv;
  std::vector<double> M(static_cast<size_t>(npe) * npe, 0.0);
  for (int q = 0; q < nq; q++) {
    const int qi[3] = {q % qv, (q / qv) % qv, q / (qv * qv)};
    double w = 1.0, J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int d = 0; d < dim; d++) w *= t.wv[qi[d]];
    for (int c = 0; c < nv; c++)
      for (int a = 0; a < dim; a++) {
        double g = 1.0;  // d/dxi_a of the multilinear shape function of corner c
        for (int d = 0; d < dim; d++) {
          const bool hi = (c >> d) & 1;
          g *= (d == a) ? (hi ? 1.0 : -1.0) : (hi ? t.xv[qi[d]] : 1.0 - t.xv[qi[d]]);
        }
        for (int i = 0; i < dim; i++) J[i][a] += g * V[c * dim + i];
      }
    const double det = dim == 2 ? J[0][0] * J[1][1] - J[0][1] * J[1][0]
                                : J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                                      J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    std::vector<double> phi(npe);
    for (int j = 0; j < npe; j++) {
      const int ji[3] = {j % n1, (j / n1) % n1, j / (n1 * n1)};
      phi[j] = 1.0;
      for (int d = 0; d < dim; d++) phi[j] *= t.Bv[qi[d] * n1 + ji[d]];
    }
    for (int j = 0; j < npe; j++)
      for (int k = 0; k < npe; k++) M[static_cast<size_t>(j) * npe + k] += w * det * phi[j] * phi[k];
  }
  double worst = 0.0;
  for (int j = 0; j < npe; j++)
    for (int k = 0; k < npe; k++) {
      double s = 0.0;
      for (int m = 0; m < npe; m++) s += M[static_cast<size_t>(j) * npe + m] * Minv[static_cast<size_t>(m) * npe + k];
      worst = std::fmax(worst, std::fabs(s - (j == k ? 1.0 : 0.0)));
    }
  return worst;
}

}  // namespace

int main() {
  for (const Row &row : table()) print_plan(row);
  const double box3[3] = {0.5, 0.2, 0.3}, box2[2] = {0.7, 0.4};
  std::printf("element_size hex %.17g\n", tpsrhs::element_sizes(element(3, box3, 0.0), 3, 1)[0]);
  std::printf("element_size quad %.17g\n", tpsrhs::element_sizes(element(2, box2, 0.0), 2, 1)[0]);
  for (int dim = 2; dim <= 3; dim++)
    for (int order = 1; order <= 2; order++) std::printf("mass_inverse_defect dim %d order %d %.3e\n", dim, order, mass_inverse_defect(dim, order));
  std::printf("OPERATOR_PLAN DONE\n");
  return 0;
}
