// libtpsrhs.so -- implementation of include/tpsrhs.h for gfx950 (MI355X).
//
// Host side: builds the face topology and the 1-D operator tables, keeps every field resident in
// HBM, and enqueues the three sweeps of kernels.hpp on one HIP stream per operator (launch.hpp).  There is no
// CPU fallback: without a HIP device tpsrhs_create returns TPSRHS_ERR_NO_DEVICE.
//
// This unit: the family loader, the parameter blocks and setup, create / destroy / mult, the setters and getters, timing,
// statuses, the two visualization entries, and the planar dry-air instantiations of the sweeps.  The other features of
// the C ABI have units of their own -- time_loop.hip, statistics.hip, sampling.hip, integrals.hip, wall_distance.hip,
// probes.hip, external_rates.hip -- and share abi_support.hpp with this one.
#include "abi_support.hpp"
#include "element_geometry.hpp"
#include "launch.hpp"
#include "operator_plan.hpp"
#include "physics_dryair.hpp"
#include "physics_dryair_axisym.hpp"
#include "physics_plasma.hpp"
#include "plasma_params_host.hpp"
#include "time_integrators.hpp"  // k_reduce_max

#include <dlfcn.h>

#include <cmath>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>

// The plasma kernel families (plasma_family.hpp) are shared objects of their own, libtpsrhs_<unit>.so next to this library,
// loaded when an operator of that family is created: load_family below.
void pick_dryair_axisym(tpsrhs_operator *op);
void pick_lte_axisym(tpsrhs_operator *op);
void pick_lte2d_axisym(tpsrhs_operator *op);
void pick_dryair_les(tpsrhs_operator *op);

TableDev upload_table(std::vector<DevBuf<void>> &owner, const tpsrhs_table &t) {
  std::vector<double> buf;
  TableDev td = table_coeffs(t, buf);
  owner.emplace_back(DevBuf<double>(buf));
  double *d = static_cast<double *>(owner.back().get());
  td.x = d;
  td.a = d + td.n;
  td.b = d + 2 * td.n;
  return td;
}

const std::vector<double> &coulomb_table_host() {
  static const std::vector<double> table = [] {
    std::vector<double> t(coulomb::SIZE);
    coll::coulomb_table_fill(t.data());
    return t;
  }();
  return table;
}

namespace {

// One shared object per plasma kernel family -- (geometry, species count, ambipolar or not, orders 1..3 or 4..5):
// libtpsrhs_plasma_<geo>_n<species>[a][_hi].so in the directory of this library, or in a directory of the colon-separated
// TPSRHS_FAMILY_PATH (development: A/B builds of one family).  dlopen'ed at the first operator that needs it and kept
// for the life of the process (the operator holds pointers to its launch functions).  The entry point is C and
// returns a status: no exception crosses the boundary.  A missing family is a loud error, never another code path, and so is
// one that was compiled against another layout of tpsrhs_operator (it exports the size it saw).
typedef int (*family_pick_fn)(tpsrhs_operator *, int, int, char *, int);
family_pick_fn load_family(const std::string &unit) {
  static std::mutex mu;
  static std::map<std::string, family_pick_fn> loaded;
  std::lock_guard<std::mutex> lock(mu);
  auto it = loaded.find(unit);
  if (it != loaded.end()) return it->second;
  std::vector<std::string> dirs;
  if (const char *env = std::getenv("TPSRHS_FAMILY_PATH")) {
    std::string e(env);
    size_t pos = 0;
    while (pos <= e.size()) {
      const size_t c = e.find(':', pos);
      const std::string d = e.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
      if (!d.empty()) dirs.push_back(d);
      if (c == std::string::npos) break;
      pos = c + 1;
    }
  }
  Dl_info info;
  if (dladdr(reinterpret_cast<const void *>(&load_family), &info) && info.dli_fname) {
    const std::string self(info.dli_fname);
    const size_t slash = self.rfind('/');
    dirs.push_back(slash == std::string::npos ? std::string(".") : self.substr(0, slash));
  }
  std::string tried;
  for (const std::string &d : dirs) {
    const std::string path = d + "/libtpsrhs_" + unit + ".so";
    if (void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL)) {
      const std::string sym = "pick_" + unit;
      // the family reads and writes the operator by its own copy of the struct: one built against another layout (a
      // leftover of a partial build, a stray TPSRHS_FAMILY_PATH) would corrupt it silently
      auto size = static_cast<const unsigned long *>(dlsym(h, (sym + "_operator_size").c_str()));
      if (!size || *size != sizeof(tpsrhs_operator)) {
        dlclose(h);
        throw Unsupported("kernel family " + unit + " was built against another operator layout: run build() (" + path + ")");
      }
      auto fn = reinterpret_cast<family_pick_fn>(dlsym(h, sym.c_str()));
      if (!fn) throw std::runtime_error(path + " does not export " + sym);
      loaded[unit] = fn;
      return fn;
    }
    const char *why = dlerror();
    tried += "\n  " + path + ": " + (why ? why : "not loadable");
  }
  throw Unsupported("kernel family " + unit + " is not available (run __graft_entry__.build()):" + tried);
}

// the parameter block of the plasma kernels (plasma_params_host.hpp) into the operator, the chemistry block to the device
template <int NSP>
void fill_plasma_params(tpsrhs_operator *op, const tpsrhs_disc *disc, const tpsrhs_physics *phys, int num_bcs,
                        const tpsrhs_bc *bcs) {
  static_assert(sizeof(PlasmaParams<NSP>) <= sizeof(op->params), "parameter block too large");
  PlasmaParams<NSP> &p = *new (op->params) PlasmaParams<NSP>;
  std::unique_ptr<ChemDev> c(new ChemDev), ext(new ChemDev);
  try {
    tpsrhs::fill_plasma_params<NSP>(p, *c, *ext, disc, phys, num_bcs, bcs, [op](const tpsrhs_table &t) { return upload_table(op->d_extra, t); });
  } catch (const UnsupportedConfig &e) {  // (its header is also built alone, on the host, by tests/host_physics: it keeps its own type)
    throw Unsupported(e.what());
  }
  op->d_chem = DevBuf<ChemDev>(1);
  p.chem = static_cast<ChemDev *>(op->d_chem.get());
  HIP_CHECK(hipMemcpy(op->d_chem.get(), c.get(), sizeof(ChemDev), hipMemcpyHostToDevice));
  // the reactions with an external rate coefficient, where there are any: a block of their own for a pass of its own
  // (external_rates.hpp); the block above does not hold them
  if (ext->num_reactions > 0) {
    op->ext.d_chem = DevBuf<ChemDev>(1);
    HIP_CHECK(hipMemcpy(op->ext.d_chem.get(), ext.get(), sizeof(ChemDev), hipMemcpyHostToDevice));
    op->ext.num_reactions = ext->num_reactions;
    op->ext.num_components_needed = external_components_needed(*ext);
  }
}

// the mixture's parameter block and the kernels of its family (the plan names the shared object)
void fill_mixture_params(tpsrhs_operator *op, const OperatorPlan &pl, const tpsrhs_disc *disc, const tpsrhs_physics *phys,
                         int num_bcs, const tpsrhs_bc *bcs) {
  switch (phys->mixture.num_species) {
    case 3:
      fill_plasma_params<3>(op, disc, phys, num_bcs, bcs);
      if (pl.coulomb_table) {  // TPSRHS_COULOMB_TABLE=0: the formulas (A/B switch within one library)
        const char *env = std::getenv("TPSRHS_COULOMB_TABLE");
        if (!env || env[0] != '0') {
          op->d_coulomb = DevBuf<double>(coulomb_table_host());
          reinterpret_cast<PlasmaParams<3> *>(op->params)->ctab = op->d_coulomb.get();
          // TPSRHS_COULOMB_WINDOW=0: every lane reads its own coefficients (the same kind of switch for the LDS window)
          const char *win = std::getenv("TPSRHS_COULOMB_WINDOW");
          reinterpret_cast<PlasmaParams<3> *>(op->params)->cwin = (!win || win[0] != '0') ? 1 : 0;
        }
      }
      break;
    case 4: fill_plasma_params<4>(op, disc, phys, num_bcs, bcs); break;
    case 5: fill_plasma_params<5>(op, disc, phys, num_bcs, bcs); break;
    case 6: fill_plasma_params<6>(op, disc, phys, num_bcs, bcs); break;
    case 7: fill_plasma_params<7>(op, disc, phys, num_bcs, bcs); break;
    default: fill_plasma_params<8>(op, disc, phys, num_bcs, bcs); break;  // MAXSPECIES of the reference's device build
  }
  char msg[512] = {0};
  const int rc = load_family(pl.unit)(op, phys->mixture.two_temperature ? 1 : 0, pl.transport, msg, static_cast<int>(sizeof msg));
  if (rc == TPSRHS_ERR_UNSUPPORTED) throw Unsupported(msg);
  if (rc == TPSRHS_ERR_INVALID_ARGUMENT) throw std::invalid_argument(msg);
  if (rc != TPSRHS_OK) throw DeviceError(msg);
}

// the tables of the table gas (the plan has checked their scales and that e(T) increases)
void upload_lte_tables(tpsrhs_operator *op, LteParams *lp, const tpsrhs_physics *phys) {
  const tpsrhs_lte &in = phys->lte;
  lp->tab_e = upload_table(op->d_extra, in.energy_table);
  lp->tab_R = upload_table(op->d_extra, in.gas_constant_table);
  lp->tab_c = upload_table(op->d_extra, in.sound_speed_table);
  tpsrhs_table rev = in.energy_table;  // "Construct e -> T table from T -> e", src/M2ulPhyS.cpp:193-200
  rev.x_data = in.energy_table.f_data;
  rev.f_data = in.energy_table.x_data;
  lp->tab_T = upload_table(op->d_extra, rev);
  {  // search aid of the inverse table: the interval of the left edge of uniform bins over the energy axis
    const int N = in.energy_table.n_data, nh = 4 * (N - 1);
    const double *ex = in.energy_table.f_data;
    const double de = (ex[N - 1] - ex[0]) / nh;
    std::vector<int> hint(nh);
    int idx = 0;
    for (int j = 0; j < nh; j++) {
      const double left = ex[0] + j * de;
      while (idx < N - 2 && ex[idx + 1] < left) idx++;
      hint[j] = idx;
    }
    op->d_extra.emplace_back(DevBuf<int>(hint));
    lp->ehint = static_cast<int *>(op->d_extra.back().get());
    lp->nhint = nh;
    lp->e0 = ex[0];
    lp->inv_de = 1.0 / de;
  }
  auto same_grid = [](const tpsrhs_table &a, const tpsrhs_table &b) {
    if (a.n_data != b.n_data || a.x_log_scale != b.x_log_scale) return 0;
    for (int k = 0; k < a.n_data; k++)
      if (a.x_data[k] != b.x_data[k]) return 0;
    return 1;
  };
  lp->thermo_same_grid = same_grid(in.energy_table, in.gas_constant_table) && same_grid(in.energy_table, in.sound_speed_table);
  lp->trans_same_grid = same_grid(in.viscosity_table, in.conductivity_table);
  lp->tab_mu = upload_table(op->d_extra, in.viscosity_table);
  lp->tab_k = upload_table(op->d_extra, in.conductivity_table);
  lp->tab_sigma = upload_table(op->d_extra, in.electric_conductivity_table);
  lp->radiation = phys->radiation.model;
  if (lp->radiation == TPSRHS_NET_EMISSION) lp->tab_nec = upload_table(op->d_extra, phys->radiation.nec_table);
}

// the two-dimensional tables of the table gas (the plan has validated them): the axes and the cell records to the device
void upload_lte2d_tables(tpsrhs_operator *op, Lte2dParams *lp, const tpsrhs_physics *phys) {
  static_cast<Lte2dTables &>(*lp) = make_lte2d_tables(phys->lte2d, [op](const void *src, size_t bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(src);
    op->d_extra.emplace_back(DevBuf<unsigned char>(std::vector<unsigned char>(b, b + bytes)));
    return static_cast<const void *>(op->d_extra.back().get());
  });
  lp->radiation = phys->radiation.model;
  if (lp->radiation == TPSRHS_NET_EMISSION) lp->tab_nec = upload_table(op->d_extra, phys->radiation.nec_table);
}

// Fluxes: sub-grid scale model and viscous sponge (src/fluxes.cpp:223-246) -> the LES flavour of the dry-air kernels
void fill_les_params(tpsrhs_operator *op, const OperatorPlan &pl, DryAirParams &d, const tpsrhs_mesh *mesh, const tpsrhs_physics *phys) {
  d.sgs_type = phys->sgs.model_type;
  d.sgs_const = pl.sgs_const;
  d.sgs_floor = phys->sgs.model_floor;
  d.vs_enabled = pl.sponge;
  for (int k = 0; k < 3; k++) {
    d.vs_n[k] = pl.sponge_n[k];
    d.vs_p[k] = pl.sponge_p[k];
  }
  d.vs_width = pl.sponge_width;
  d.vs_ratio = pl.sponge_ratio;
  const Topology &tp = op->topo;
  std::vector<double> delta = mesh->elem_size ? std::vector<double>(mesh->elem_size, mesh->elem_size + tp.ne)
                                              : element_sizes(tp.verts, op->dim, tp.ne);
  for (double &v : delta) v /= op->order;  // elSize = GetElementSize(e, 1) / order, src/rhs_operator.cpp:154
  op->d_extra.emplace_back(DevBuf<double>(delta));
  d.elem_delta = static_cast<double *>(op->d_extra.back().get());
}

// the dry-air block, which the table gas extends (boundary conditions and switches are shared)
void fill_single_fluid_params(tpsrhs_operator *op, const OperatorPlan &pl, const tpsrhs_mesh *mesh, const tpsrhs_disc *disc,
                              const tpsrhs_physics *phys, int num_bcs, const tpsrhs_bc *bcs) {
  static_assert(sizeof(LteParams) <= sizeof(op->params) && sizeof(Lte2dParams) <= sizeof(op->params), "parameter block");
  LteParams *lp = (pl.lte && !pl.lte2d) ? new (op->params) LteParams : nullptr;
  if (lp) std::memset(static_cast<void *>(lp), 0, sizeof(LteParams));
  Lte2dParams *lp2 = pl.lte2d ? new (op->params) Lte2dParams : nullptr;
  if (lp2) std::memset(static_cast<void *>(lp2), 0, sizeof(Lte2dParams));
  DryAirParams &d = lp ? *static_cast<DryAirParams *>(lp) : (lp2 ? *static_cast<DryAirParams *>(lp2) : *new (op->params) DryAirParams);
  if (!lp && !lp2) std::memset(&d, 0, sizeof(d));
  if (lp) upload_lte_tables(op, lp, phys);
  if (lp2) upload_lte2d_tables(op, lp2, phys);
  d.gamma = phys->dry_air.specific_heat_ratio;
  d.Rg = phys->dry_air.gas_constant;
  d.inv_Rg = 1.0 / d.Rg;
  d.visc_mult = phys->dry_air.visc_mult;
  d.bulk_mult = phys->dry_air.bulk_visc_mult;
  d.C1 = phys->dry_air.sutherland_C1;
  d.S0 = phys->dry_air.sutherland_S0;
  d.cp_div_pr = d.gamma * d.Rg / (phys->dry_air.sutherland_Pr * (d.gamma - 1.0));
  d.eq_system = phys->eq_system;
  d.use_bc_in_grad = disc->use_bc_in_grad;
  d.use_roe = disc->use_roe ? 1 : 0;
  d.ref_length = disc->ref_length > 0.0 ? disc->ref_length : 1.0;  // config.refLength default, run_configuration.cpp:66
  d.num_bcs = num_bcs;
  for (int i = 0; i < num_bcs; i++) {
    d.bc[i].category = bcs[i].category;
    d.bc[i].type = bcs[i].type;
    for (int k = 0; k < 4 + TPSRHS_MAXSPECIES; k++) d.bc[i].data[k] = bcs[i].data[k];
  }
  if (pl.les) fill_les_params(op, pl, d, mesh, phys);
}

// vertices, face table and, for the non-collocated pair, the inverse mass matrices
void upload_geometry(tpsrhs_operator *op) {
  const Topology &tp = op->topo;
  op->d_verts = DevBuf<double>(tp.verts);
  if (op->nc) op->d_minv = DevBuf<double>(inverse_mass_matrices(tp.verts, op->dim, op->order, op->ne));
  std::vector<int2> fi(tp.face_nbr.size());
  for (size_t i = 0; i < fi.size(); i++) fi[i] = make_int2(tp.face_nbr[i], tp.face_orient[i]);
  op->d_face_info = DevBuf<int2>(fi);
}

// faces of the non-reflecting patches (dry air), in slot order, and the state they carry from one Mult to the next
void build_nr_tables(tpsrhs_operator *op, const tpsrhs_bc *bcs) {
  const Topology &tp = op->topo;
  std::vector<int2> nrf;
  std::vector<int> ordinal(tp.face_nbr.size(), -1);
  DryAirParams &d = *reinterpret_cast<DryAirParams *>(op->params);
  for (size_t slot = 0; slot < tp.face_nbr.size(); slot++) {
    const int nb = tp.face_nbr[slot];
    if (nb >= 0) continue;
    const int b = -nb - 1;
    if (!is_non_reflecting(bcs[b].category, bcs[b].type)) continue;
    ordinal[slot] = static_cast<int>(nrf.size());
    nrf.push_back(make_int2(static_cast<int>(slot), b));
    // tangent1 of the patch: the caller's (the reference takes it from its first boundary face,
    // src/outletBC.cpp:160-172) or an edge of our first face of the patch, orthogonalised to nothing --
    // as there, the patch is assumed planar
    double *t1 = &d.bc[b].data[4];
    if (t1[0] == 0.0 && t1[1] == 0.0 && t1[2] == 0.0) {
      const int e = static_cast<int>(slot) / op->nfaces, lf = static_cast<int>(slot) % op->nfaces, D = lf >> 1, sd = lf & 1;
      const int nv = 1 << op->dim, a = (op->dim == 2) ? 1 - D : (D == 0 ? 1 : 0);
      const int c0 = sd << D, c1 = c0 | (1 << a);
      double mod = 0.0, t[3] = {0, 0, 0};
      for (int k = 0; k < op->dim; k++) {
        t[k] = tp.verts[(static_cast<size_t>(e) * nv + c1) * op->dim + k] - tp.verts[(static_cast<size_t>(e) * nv + c0) * op->dim + k];
        mod += t[k] * t[k];
      }
      for (int k = 0; k < 3; k++) t1[k] = t[k] / std::sqrt(mod);
    }
  }
  if (tp.num_shared > 0 && !op->reduce)
    throw HaloError("halo: a partitioned mesh with non-reflecting patches needs runtime.reduce");
  op->n_nr_faces = static_cast<int>(nrf.size());
  op->d_bc_sums = DevBuf<double>(MAXBC * (TPSRHS_MAXEQUATIONS + 1));
  HIP_CHECK(hipMemset(op->d_bc_sums.get(), 0, MAXBC * (TPSRHS_MAXEQUATIONS + 1) * sizeof(double)));
  if (nrf.empty()) return;
  op->d_nr_faces = DevBuf<int2>(nrf);
  op->d_nr_ordinal = DevBuf<int>(ordinal);
  const size_t n = nrf.size() * static_cast<size_t>(op->nq) * op->neq;
  for (int k = 0; k < 2; k++) {
    op->d_bstate[k] = DevBuf<double>(n);
    HIP_CHECK(hipMemset(op->d_bstate[k].get(), 0, n * sizeof(double)));
  }
}

// the fields every Mult works in, and the send buffer and offsets of a partitioned mesh
void allocate_work_buffers(tpsrhs_operator *op) {
  const Topology &tp = op->topo;
  if (op->ndofs >= (int64_t(1) << 31)) throw Unsupported("more than 2^31 nodes per rank");
  const int64_t nslots = static_cast<int64_t>(op->ne) * op->nfaces + tp.num_shared;
  op->d_Up = DevBuf<double>(op->neq * op->ndofs);
  op->d_gradUp = DevBuf<double>(op->dim * op->neq * op->ndofs);
  op->d_TA = DevBuf<double>(nslots * 2 * op->neq * op->nf);
  op->d_TB = DevBuf<double>(nslots * (op->neq - 1) * op->nq);
  HIP_CHECK(hipMemset(op->d_TA.get(), 0, nslots * 2 * op->neq * op->nf * sizeof(double)));
  HIP_CHECK(hipMemset(op->d_TB.get(), 0, nslots * (op->neq - 1) * op->nq * sizeof(double)));
  op->d_speed = DevBuf<double>(1);
  HIP_CHECK(hipMemset(op->d_speed.get(), 0, sizeof(double)));
  if (tp.num_shared > 0) {
    op->d_shared_slot = DevBuf<int32_t>(tp.shared_slot);
    op->d_shared_orient = DevBuf<uint8_t>(tp.shared_orient);
    const int64_t per0 = 2 * op->neq * op->nf, per1 = static_cast<int64_t>(op->neq - 1) * op->nq;
    op->d_send = DevBuf<double>(tp.num_shared * std::max(per0, per1));
    for (size_t i = 0; i < tp.nbr_offsets.size(); i++) {
      op->send_off[0].push_back(tp.nbr_offsets[i] * per0);
      op->send_off[1].push_back(tp.nbr_offsets[i] * per1);
    }
    op->recv_off[0] = op->send_off[0];
    op->recv_off[1] = op->send_off[1];
  }
}

// operator_plan.hpp keeps host copies of two predicates of the device headers: they agree on every (category, type) of
// the public enums (checked once per process, at the first tpsrhs_create)
static_assert(PLAN_MAXBC == MAXBC && PLAN_PLASMA_MAXBC == PLASMA_MAXBC, "operator_plan.hpp: boundary-condition limits");
static_assert(PLAN_TRANSPORT_CONSTANT == TRANSPORT_CONSTANT && PLAN_TRANSPORT_ARGON_MINIMAL == TRANSPORT_ARGON_MINIMAL &&
                  PLAN_TRANSPORT_ARGON_MIXTURE == TRANSPORT_ARGON_MIXTURE, "operator_plan.hpp: transport indices");
bool plan_predicates_agree() {
  for (int cat = TPSRHS_INLET; cat <= TPSRHS_WALL; cat++)
    for (int type = 0; type <= TPSRHS_SUB_VEL_CONST_ENT; type++)
      if (plan_is_non_reflecting(cat, type) != is_non_reflecting(cat, type) || plan_is_face_inlet(cat, type) != is_face_inlet(cat, type))
        return false;
  return true;
}

// plan (operator_plan.hpp: every refusal that needs neither a device nor the mesh) -> device -> topology -> parameter block
// and kernels -> geometry -> non-reflecting tables -> work buffers -> timing events
void setup(tpsrhs_operator *op, const tpsrhs_mesh *mesh, const tpsrhs_disc *disc, const tpsrhs_physics *phys,
           int num_bcs, const tpsrhs_bc *bcs, const tpsrhs_runtime *rt) {
  static const bool agree = plan_predicates_agree();
  if (!agree) throw std::logic_error("operator_plan.hpp and the device headers disagree about a boundary-condition predicate");
  const OperatorPlan pl = plan_operator(mesh->dim, *disc, *phys, num_bcs, bcs);
  op->nc = pl.nc;
  op->dim = pl.dim;
  op->order = pl.order;
  op->nvel = pl.nvel;
  op->neq = pl.neq;
  op->phys = *phys;

  require_device("no HIP device visible; tpsrhs has no CPU path");
  op->device = rt ? rt->device : 0;
  HIP_CHECK(hipSetDevice(op->device));
  op->stream = rt ? static_cast<hipStream_t>(rt->stream) : nullptr;
  if (const char *env = std::getenv("TPSRHS_SWEEP_ALT")) op->loop.sweep_alt = env[0] != '0';  // (A/B switch; default on)
  if (const char *env = std::getenv("TPSRHS_FUSE_TRACES")) op->loop.chain.set_fusing(env[0] != '0');  // (A/B switch; default on)
  op->loop.sp_first = pl.sp_first;
  op->loop.sp_last = pl.sp_last;
  op->halo = rt ? rt->halo : nullptr;
  op->halo_ctx = rt ? rt->halo_ctx : nullptr;
  op->reduce = rt ? rt->reduce : nullptr;
  op->reduce_ctx = rt ? rt->reduce_ctx : nullptr;

  op->topo = build_topology(*mesh, num_bcs, bcs);
  const Topology &tp = op->topo;
  if (tp.num_shared > 0 && !op->halo) throw std::invalid_argument("mesh has shared faces but runtime.halo is NULL");
  op->ne = tp.ne;
  op->nfaces = tp.nfaces;
  const int n1 = op->order + 1, q1 = rule_points(op->nc, (op->dim - 1) + 2 * op->order);
  op->nf = (op->dim == 3) ? n1 * n1 : n1;
  op->nq = (op->dim == 3) ? q1 * q1 : q1;
  const int npe = (op->dim == 3) ? n1 * n1 * n1 : n1 * n1;
  op->ndofs = static_cast<int64_t>(op->ne) * npe;

  if (pl.heavy2d && pl.sponge) {  // the plane travels in MeshDev, the closures scale their coefficients (src/fluxes.cpp:232-246)
    op->vs2d.enabled = 1;
    for (int k = 0; k < 2; k++) {
      op->vs2d.n[k] = pl.sponge_n[k];
      op->vs2d.p[k] = pl.sponge_p[k];
    }
    op->vs2d.width = pl.sponge_width;
    op->vs2d.ratio = pl.sponge_ratio;
  }
  if (pl.plasma) {
    fill_mixture_params(op, pl, disc, phys, num_bcs, bcs);
  } else {
    fill_single_fluid_params(op, pl, mesh, disc, phys, num_bcs, bcs);
    if (pl.les)
      pick_dryair_les(op);
    else if (pl.lte2d)
      pick_lte2d_axisym(op);
    else if (pl.lte)
      pick_lte_axisym(op);
    else if (disc->axisymmetric)
      pick_dryair_axisym(op);
    else if (op->dim == 3)
      pl.any_nr ? pick_order<3, DryAirPhys<3, true>>(op) : pick_order<3, DryAirPhys<3>>(op);
    else
      pl.any_nr ? pick_order<2, DryAirPhys<2, true>>(op) : pick_order<2, DryAirPhys<2>>(op);
  }
  upload_geometry(op);
  if (pl.any_nr) build_nr_tables(op, bcs);
  op->has_nr = pl.any_nr;
  allocate_work_buffers(op);
  for (auto &set : op->evs)
    for (auto &e : set) HIP_CHECK(hipEventCreate(&e));
}


}  // namespace

#if TPSRHS_STAMP
// diagnostic builds of this unit (-DTPSRHS_STAMP=1 / 2, tools/stamp_phases.py with a dry-air workload): the phase cycles of
// the first `nblocks` blocks of the last stamped kernel
extern "C" int tpsrhs_debug_stamps(unsigned int *out, int nblocks) {
  const size_t bytes = static_cast<size_t>(nblocks) * tpsrhs::NSTAMP * sizeof(unsigned int);
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(tpsrhs::g_stamp), bytes) == hipSuccess ? 0 : 1;
}
#endif

extern "C" {

int tpsrhs_create(const tpsrhs_mesh *mesh, const tpsrhs_disc *disc, const tpsrhs_physics *physics, int num_bcs,
                  const tpsrhs_bc *bcs, const tpsrhs_runtime *runtime, tpsrhs_handle *out) {
  if (!mesh || !disc || !physics || !out || (num_bcs > 0 && !bcs))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_create: NULL argument");
  *out = nullptr;
  std::unique_ptr<tpsrhs_operator> op(new tpsrhs_operator());
  const int st = guarded([&] { setup(op.get(), mesh, disc, physics, num_bcs, bcs, runtime); });
  if (st == TPSRHS_OK) *out = op.release();
  return st;
}

int tpsrhs_destroy(tpsrhs_handle h) {
  if (!h) return TPSRHS_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a sample, a record or a reduction may still be running
  transfer_forget(h);
  delete h;
  return TPSRHS_OK;
}

int tpsrhs_mult(tpsrhs_handle h, const double *x, double *y, double /*time*/, double *max_char_speed) {
  if (!h || !x || !y) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_mult: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    h->launch(h, x, y, false);
    if (max_char_speed) {
      hipLaunchKernelGGL(k_reduce_max<1024>, dim3(1), dim3(1024), 0, h->stream, h->flux_grid, h->d_block_speed.get(), h->d_speed.get());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(max_char_speed, h->d_speed.get(), sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipStreamSynchronize(h->stream));
    }
  });
}

int tpsrhs_mult_host(tpsrhs_handle h, const double *x, double *y, double time, double *max_char_speed) {
  if (!h || !x || !y) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_mult_host: NULL argument");
  const size_t bytes = static_cast<size_t>(h->neq) * h->ndofs * sizeof(double);
  int st = guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (!h->d_xh) {
      h->d_xh = DevBuf<double>(h->neq * h->ndofs);
      h->d_yh = DevBuf<double>(h->neq * h->ndofs);
    }
    HIP_CHECK(hipMemcpyAsync(h->d_xh.get(), x, bytes, hipMemcpyHostToDevice, h->stream));
  });
  if (st != TPSRHS_OK) return st;
  st = tpsrhs_mult(h, h->d_xh.get(), h->d_yh.get(), time, max_char_speed);
  if (st != TPSRHS_OK) return st;
  return guarded([&] {
    HIP_CHECK(hipMemcpyAsync(y, h->d_yh.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

int tpsrhs_set_dt(tpsrhs_handle h, double dt) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_dt: NULL handle");
  h->nr_dt = dt;
  return TPSRHS_OK;
}

namespace {
void upload_forcing(tpsrhs_operator *h) {
  const ForcingDev &f = h->forcing;
  h->forcing_terms = f.has_pg || f.nheat > 0 || f.nsponge > 0 || f.nps > 0 || f.joule != nullptr;
  h->forcing_active = h->forcing_terms || h->ext.rates != nullptr;
  if (!h->forcing_terms) return;
  HIP_CHECK(hipSetDevice(h->device));
  if (!h->d_forcing) h->d_forcing = DevBuf<ForcingDev>(1);
  HIP_CHECK(hipStreamSynchronize(h->stream));  // an earlier Mult may still read the block
  HIP_CHECK(hipMemcpy(h->d_forcing.get(), &h->forcing, sizeof(ForcingDev), hipMemcpyHostToDevice));
}
}  // namespace

int tpsrhs_set_forcing(tpsrhs_handle h, const tpsrhs_forcing *in) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_forcing: NULL handle");
  return guarded([&] {
    ForcingDev f = {};
    f.joule = h->forcing.joule;
    // plane-node lists and sum buffers of the mixed-out zones of THIS call; swapped with the previous call's once the new
    // block is in place, so that whichever set is no longer in force is freed at the end of this scope (these, if the
    // call fails: the old forcing then stays as it was)
    std::vector<DevBuf<void>> mixed_out;
    if (in) {
      if (in->num_heat_sources < 0 || in->num_heat_sources > TPSRHS_MAXHEATSOURCES || in->num_sponge_zones < 0 ||
          in->num_sponge_zones > TPSRHS_MAXSPONGEZONES)
        throw std::invalid_argument("tpsrhs_set_forcing: heat source / sponge zone count out of range");
      if (in->num_passive_scalars < 0 || in->num_passive_scalars > TPSRHS_MAXPASSIVESCALARS)
        throw std::invalid_argument("tpsrhs_set_forcing: passive scalar count out of range");
      f.nps = in->num_passive_scalars;
      for (int i = 0; i < f.nps; i++) {  // PassiveScalar constructor, src/forcing_terms.cpp:778-790
        const tpsrhs_passive_scalar &s = in->passive_scalars[i];
        if (!(s.radius > 0.0)) throw std::invalid_argument("tpsrhs_set_forcing: passive scalar radius must be positive");
        for (int d = 0; d < 3; d++) f.ps[i].x0[d] = s.coords[d];
        f.ps[i].radius = s.radius;
        f.ps[i].value = s.value;
      }
      const int dim = h->dim;
      f.has_pg = in->has_pressure_gradient ? 1 : 0;
      for (int d = 0; d < 3; d++) f.pg[d] = in->pressure_gradient[d];
      f.nheat = in->num_heat_sources;
      for (int i = 0; i < f.nheat; i++) {  // HeatSource constructor, src/forcing_terms.cpp:890-899
        const tpsrhs_heat_source &s = in->heat_sources[i];
        ForcingDev::Heat &d = f.heat[i];
        d.value = s.value;
        d.radius = s.radius;
        double mod = 0.0;
        for (int k = 0; k < dim; k++) mod += (s.point2[k] - s.point1[k]) * (s.point2[k] - s.point1[k]);
        mod = std::sqrt(mod);
        if (!(mod > 0.0)) throw std::invalid_argument("tpsrhs_set_forcing: heat source with point1 == point2");
        d.len = mod;
        for (int k = 0; k < 3; k++) {
          d.p1[k] = s.point1[k];
          d.axis[k] = k < dim ? (s.point2[k] - s.point1[k]) / mod : 0.0;
        }
      }
      f.nsponge = in->num_sponge_zones;
      for (int i = 0; i < f.nsponge; i++) {
        const tpsrhs_sponge_zone &s = in->sponge_zones[i];
        ForcingDev::Sponge &d = f.sponge[i];
        if (s.type != TPSRHS_SPONGE_PLANAR && s.type != TPSRHS_SPONGE_ANNULUS)
          throw std::invalid_argument("tpsrhs_set_forcing: unknown sponge zone type");
        if (s.type == TPSRHS_SPONGE_ANNULUS && dim != 3)
          throw Unsupported("annular sponge zone needs dim == 3 (the reference's transform indexes 3 components)");
        d.type = s.type;
        double mod = 0.0;  // "make sure normal is unitary", src/forcing_terms.cpp:528-532
        for (int k = 0; k < dim; k++) mod += s.normal[k] * s.normal[k];
        mod = std::sqrt(mod);
        if (!(mod > 0.0)) throw std::invalid_argument("tpsrhs_set_forcing: sponge zone with a zero normal");
        for (int k = 0; k < 3; k++) {
          d.normal[k] = k < dim ? s.normal[k] / mod : 0.0;
          d.p0[k] = s.point0[k];
          d.pinit[k] = s.point_init[k];
        }
        d.r1 = s.r1;
        d.r2 = s.r2;
        d.mult = s.mult_factor;
        if (s.solution_type == TPSRHS_SPONGE_MIXEDOUT) {
          // nodesInMixedOutPlane of the constructor, src/forcing_terms.cpp:553-606
          if (h->phys.working_fluid != TPSRHS_DRY_AIR || h->nvel != dim)
            throw Unsupported("mixed-out sponge zone: built for dry air, planar 2-D and 3-D");
          if (!(s.tol > 0.0)) throw std::invalid_argument("tpsrhs_set_forcing: mixed-out sponge zone needs tol > 0");
          const Tables1D t = make_tables(h->order, dim, h->nc, h->nc);
          const int n1 = h->order + 1, npe = (dim == 3) ? n1 * n1 * n1 : n1 * n1, nv = 1 << dim;
          std::vector<int> nodes;
          for (int e = 0; e < h->ne; e++) {
            const double *V = &h->topo.verts[static_cast<size_t>(e) * nv * dim];
            for (int k = 0; k < npe; k++) {
              const int idx[3] = {k % n1, (k / n1) % n1, k / (n1 * n1)};
              double X[3] = {0.0, 0.0, 0.0};
              for (int v = 0; v < nv; v++) {
                double shp = 1.0;
                for (int a = 0; a < dim; a++) shp *= ((v >> a) & 1) ? t.x[idx[a]] : 1.0 - t.x[idx[a]];
                for (int i = 0; i < dim; i++) X[i] += shp * V[v * dim + i];
              }
              double dist_init = 0.0;
              for (int a = 0; a < dim; a++) dist_init -= d.normal[a] * (X[a] - d.pinit[a]);
              bool in_plane;
              if (d.type == TPSRHS_SPONGE_PLANAR) {
                in_plane = std::fabs(dist_init) < s.tol;
              } else {
                double R = 0.0;
                for (int a = 0; a < dim; a++) {
                  const double tt = X[a] - d.pinit[a] + dist_init * d.normal[a];
                  R += tt * tt;
                }
                in_plane = std::fabs(std::sqrt(R) - d.r1) < s.tol;
              }
              if (in_plane) nodes.push_back(e * npe + k);
            }
          }
          if (nodes.empty() && h->topo.num_shared == 0)
            throw std::invalid_argument("tpsrhs_set_forcing: no node within tol of the mix-out plane");
          // the plane sums are added over the ranks (MPI_Allreduce of src/forcing_terms.cpp:732-735): without the hook a
          // partitioned run would use rank-local means, and a rank without plane nodes 0 / 0
          if (h->topo.num_shared > 0 && !h->reduce)
            throw std::invalid_argument("tpsrhs_set_forcing: a mixed-out sponge zone on a partitioned mesh needs runtime.reduce");
          d.mixed_out = 1;
          d.n_plane = static_cast<int>(nodes.size());
          DevBuf<int> dn(nodes);
          DevBuf<double> ds(TPSRHS_MAXEQUATIONS + 1);
          d.plane_nodes = dn.get();
          d.msum = ds.get();
          mixed_out.emplace_back(std::move(dn));
          mixed_out.emplace_back(std::move(ds));
          for (int eq = 0; eq < TPSRHS_MAXEQUATIONS; eq++) d.target[eq] = 0.0;
        } else {
          if (s.solution_type != TPSRHS_SPONGE_USERDEF) throw std::invalid_argument("tpsrhs_set_forcing: unknown sponge solution type");
          for (int eq = 0; eq < TPSRHS_MAXEQUATIONS; eq++) d.target[eq] = eq < h->neq ? s.target_U[eq] : 0.0;
          if (!(d.target[0] > 0.0)) throw std::invalid_argument("tpsrhs_set_forcing: sponge target density must be positive");
        }
      }
    }
    // the device block first; the host copy, the buffers of the mixed-out zones and the configuration epoch are committed
    // only once it is in place -- if the upload fails the operator keeps its previous forcing and its buffers
    const ForcingDev prev = h->forcing;
    const bool prev_active = h->forcing_active, prev_terms = h->forcing_terms;
    h->forcing = f;
    {
      ScopeExit rollback([&](bool failed) {
        if (failed) {
          h->forcing = prev;
          h->forcing_active = prev_active;
          h->forcing_terms = prev_terms;
        }
      });
      upload_forcing(h);  // synchronises the stream before it overwrites the device block
      HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    h->d_mixed_out.swap(mixed_out);
    h->loop.config_epoch++;
  });
}

int tpsrhs_set_mixing_length(tpsrhs_handle h, const double *distance, const tpsrhs_mixing_length *in) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_mixing_length: NULL handle");
  return guarded([&] {
    if (distance) {
      if (!in) throw std::invalid_argument("tpsrhs_set_mixing_length: parameters missing");
      // the 2-D kernels with the `heavy` closure interface: mixtures (planar, axisymmetric), axisymmetric dry air
      const bool plasma = h->phys.working_fluid == TPSRHS_USER_DEFINED;
      if (h->dim != 2 || !(plasma || h->nvel == 3))
        throw Unsupported("mixing-length model: built for the 2-D kernels (mixtures planar / axisymmetric, dry air axisymmetric)");
      if (h->nc) throw Unsupported("mixing-length model: Gauss-Legendre pair");
      if (!(in->max_mixing_length >= 0.0)) throw std::invalid_argument("tpsrhs_set_mixing_length: negative max_mixing_length");
      h->mixlen.distance = distance;
      h->mixlen.lmax = in->max_mixing_length;
      h->mixlen.prt = in->pr_ratio;
      h->mixlen.bulk = in->bulk_multiplier;
    } else {
      h->mixlen.distance = nullptr;
    }
    h->loop.config_epoch++;  // a captured time-loop graph holds the old pointer
  });
}

int tpsrhs_set_joule_heating(tpsrhs_handle h, const double *joule_heating) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_joule_heating: NULL handle");
  return guarded([&] {
    // JouleHeating::updateTerms asserts nvel == 3 (src/forcing_terms.cpp:444)
    if (joule_heating && h->nvel != 3) throw Unsupported("JouleHeating needs three velocity components (3-D or axisymmetric)");
    h->forcing.joule = joule_heating;
    h->loop.config_epoch++;
    upload_forcing(h);
  });
}

int tpsrhs_update_gradients(tpsrhs_handle h, const double *x) {
  if (!h || !x) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_update_gradients: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    h->launch(h, x, nullptr, true);
  });
}

int tpsrhs_get_primitives(tpsrhs_handle h, double *up_out) {
  if (!h || !up_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_get_primitives: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipMemcpyAsync(up_out, h->d_Up.get(), sizeof(double) * h->neq * h->ndofs, hipMemcpyDeviceToDevice, h->stream));
  });
}

int tpsrhs_get_gradients(tpsrhs_handle h, double *gradup_out) {
  if (!h || !gradup_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_get_gradients: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipMemcpyAsync(gradup_out, h->d_gradUp.get(), sizeof(double) * h->dim * h->neq * h->ndofs,
                             hipMemcpyDeviceToDevice, h->stream));
  });
}

int64_t tpsrhs_height(tpsrhs_handle h) { return h ? h->neq * h->ndofs : -1; }
int64_t tpsrhs_num_dofs(tpsrhs_handle h) { return h ? h->ndofs : -1; }
int tpsrhs_num_equation(tpsrhs_handle h) { return h ? h->neq : -1; }

int tpsrhs_enable_kernel_timing(tpsrhs_handle h, int enable) {
  if (!h) return TPSRHS_ERR_INVALID_ARGUMENT;
  h->timing = enable != 0;
  h->sets_recorded = 0;
  return TPSRHS_OK;
}

int tpsrhs_kernel_times(tpsrhs_handle h, int capacity, const char **names, double *milliseconds) {
  if (!h || h->sets_recorded == 0) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  const int nsets = static_cast<int>(std::min<int64_t>(h->sets_recorded, tpsrhs_operator::MAXSETS));
  int n = 0;
  for (int k = 0; k < NKERN && n < capacity; k++, n++) {
    double sum = 0.0;
    for (int i = 0; i < nsets; i++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->evs[i][k], h->evs[i][k + 1]) != hipSuccess) return n;
      sum += ms;
    }
    if (names) names[n] = kKernelNames[k];
    if (milliseconds) milliseconds[n] = sum / nsets;  // average over the recorded Mults
  }
  return n;
}

int tpsrhs_eval_pointwise(tpsrhs_handle h, int quantity, int64_t n, const double *U, double *out) {
  if (!h || n < 0 || !U || !out || quantity < 0 || quantity > 3) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "eval_pointwise");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    h->point_eval(h, quantity, n, U, out);
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

int tpsrhs_mult_times(tpsrhs_handle h, int capacity, double *milliseconds) {
  if (!h || h->sets_recorded == 0 || !milliseconds) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  const int nsets = static_cast<int>(std::min<int64_t>(h->sets_recorded, tpsrhs_operator::MAXSETS));
  int n = 0;
  for (; n < nsets && n < capacity; n++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->evs[n][0], h->evs[n][NKERN]) != hipSuccess) return n;
    milliseconds[n] = ms;
  }
  return n;
}

int tpsrhs_kernel_bytes(tpsrhs_handle h, int capacity, const char **names, double *bytes) {
  if (!h) return 0;
  // algorithmic HBM traffic of the three sweeps ("bytes per unit"), in bytes per Mult
  const double N = static_cast<double>(h->ndofs), neq = h->neq, dim = h->dim;
  const double slots = static_cast<double>(h->ne) * h->nfaces;
  const double ta = slots * 2 * neq * h->nf, tb = slots * (neq - 1) * h->nq;
  const double geo = static_cast<double>(h->ne) * (1 << h->dim) * dim;
  const double b[NKERN] = {
      8.0 * (neq * N /*U*/ + ta),
      8.0 * (neq * N + 0.5 * ta /*neighbour Up traces*/ + neq * N /*Up*/ + dim * neq * N /*gradUp*/ + tb + geo),
      8.0 * (neq * N + dim * neq * N + 0.5 * ta /*neighbour U traces*/ + 2.0 * tb + neq * N /*y*/ + geo)};
  int n = 0;
  for (int k = 0; k < NKERN && n < capacity; k++, n++) {
    if (names) names[n] = kKernelNames[k];
    if (bytes) bytes[n] = b[k];
  }
  return n;
}

int tpsrhs_face_tables(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int32_t *face_nbr,
                       uint8_t *face_orient, int32_t *shared_slot, uint8_t *shared_orient) {
  if (!mesh || !face_nbr || !face_orient) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_face_tables: NULL argument");
  return guarded([&] {
    const Topology T = build_topology(*mesh, num_bcs, bcs);
    std::memcpy(face_nbr, T.face_nbr.data(), T.face_nbr.size() * sizeof(int32_t));
    std::memcpy(face_orient, T.face_orient.data(), T.face_orient.size());
    if (shared_slot && T.num_shared) std::memcpy(shared_slot, T.shared_slot.data(), T.num_shared * sizeof(int32_t));
    if (shared_orient && T.num_shared) std::memcpy(shared_orient, T.shared_orient.data(), T.num_shared);
  });
}

const char *tpsrhs_status_string(int status) {
  switch (status) {
    case TPSRHS_OK: return "TPSRHS_OK";
    case TPSRHS_ERR_INVALID_ARGUMENT: return "TPSRHS_ERR_INVALID_ARGUMENT";
    case TPSRHS_ERR_UNSUPPORTED: return "TPSRHS_ERR_UNSUPPORTED";
    case TPSRHS_ERR_MESH: return "TPSRHS_ERR_MESH";
    case TPSRHS_ERR_DEVICE: return "TPSRHS_ERR_DEVICE";
    case TPSRHS_ERR_NO_DEVICE: return "TPSRHS_ERR_NO_DEVICE";
    case TPSRHS_ERR_HALO: return "TPSRHS_ERR_HALO";
    default: return "TPSRHS_ERR_UNKNOWN";
  }
}
const char *tpsrhs_last_error(void) { return last_error().c_str(); }
int tpsrhs_get_plasma_conductivity(tpsrhs_handle h, const double *x, double *sigma_out) {
  if (!h || !x || !sigma_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_get_plasma_conductivity: NULL argument");
  return guarded([&] {
    if (h->phys.working_fluid == TPSRHS_DRY_AIR) throw Unsupported("plasma conductivity output: dry air has no SourceTerm");
    if (h->phys.working_fluid == TPSRHS_USER_DEFINED && !h->phys.mixture.ambipolar && h->phys.chemistry.num_reactions > 0)
      throw Unsupported("plasma conductivity output: the reference's SourceTerm does not store it for a reacting mixture that "
                        "is not ambipolar (src/source_term.cpp:178-197)");
    HIP_CHECK(hipSetDevice(h->device));
    h->point_eval(h, 4, h->ndofs, x, sigma_out);
  });
}

const char *tpsrhs_version(void) { return "tpsrhs 0.1.0 (gfx950)"; }

}  // extern "C"

// =============================================================================================
// Plasma post-processing fields (visualization.hpp): M2ulPhyS::updateVisualizationVariables on the device.  No kernel of
// this unit: the passes live in shared objects of their own (plasma_vis_family.hpp), loaded at the first call and reached
// through tpsrhs_operator::vis_fields.
// =============================================================================================
namespace {
int vis_layout(const tpsrhs_physics &ph, int dim, int axisymmetric, tpsrhs_vis_layout *out) {
  if (ph.working_fluid == TPSRHS_DRY_AIR)
    throw Unsupported("visualization fields: dry air has none (the reference skips the block, src/M2ulPhyS.cpp:4199)");
  if (ph.working_fluid != TPSRHS_USER_DEFINED)
    throw Unsupported("visualization fields: built for the species mixtures (fluid = user_defined), not for the table gas");
  const int nsp = ph.mixture.num_species, R = ph.chemistry.num_reactions;
  if (nsp < 1 || nsp > TPSRHS_MAXSPECIES) throw std::invalid_argument("tpsrhs_visualization_layout: num_species");
  if (R < 0 || R > TPSRHS_MAXREACTIONS) throw std::invalid_argument("tpsrhs_visualization_layout: num_reactions");
  const int nvel = (axisymmetric || dim == 3) ? 3 : 2;
  tpsrhs_vis_layout l;
  l.num_species = nsp;
  l.nvel = nvel;
  l.num_reactions = R;
  int row = 0;  // the registration order of src/M2ulPhyS.cpp:1690-1787
  l.Xsp = row, row += nsp;
  l.Ysp = row, row += nsp;
  l.nsp_ = row, row += nsp;
  l.FluxTrns = row, row += 4;         // FluxTrns::NUM_FLUX_TRANS
  l.diffVel = row, row += nsp * nvel;
  l.SrcTrns = row, row += 1;          // SrcTrns::NUM_SRC_TRANS
  l.SpeciesTrns = row, row += nsp;    // SpeciesTrns::NUM_SPECIES_COEFFS = 1
  l.rxn = R > 0 ? row : -1, row += R;
  l.nrows = row;
  *out = l;
  return row;
}
}  // namespace

// the per-node passes of the operator's family (plasma_vis_family.hpp): a shared object of its own, loaded at the first call
// that needs one of them; sets vis_fields, ext_reactions and boltzmann_fields
void load_plasma_vis_family(tpsrhs_operator *h, const char *who) {
  if (h->vis_fields) return;
  const tpsrhs_perfect_mixture &mx = h->phys.mixture;
  const int tr = (h->phys.transport_model == TPSRHS_CONSTANT)
                     ? TRANSPORT_CONSTANT
                     : (h->phys.transport_model == TPSRHS_ARGON_MINIMAL ? TRANSPORT_ARGON_MINIMAL : TRANSPORT_ARGON_MIXTURE);
  const char *geo = (h->dim == 3) ? "3d" : (h->nvel > h->dim ? "axi" : "2d");
  const std::string unit = std::string("plasma_vis_") + geo + "_n" + std::to_string(mx.num_species) + (mx.ambipolar ? "a" : "");
  char msg[512] = {0};
  const int rc = load_family(unit)(h, mx.two_temperature ? 1 : 0, tr, msg, static_cast<int>(sizeof msg));
  if (rc != TPSRHS_OK || !h->vis_fields || !h->ext_reactions || !h->boltzmann_fields) throw Unsupported(std::string(who) + ": " + msg);
}

extern "C" {

int tpsrhs_visualization_layout(const tpsrhs_physics *physics, int dim, int axisymmetric, tpsrhs_vis_layout *out) {
  if (!physics || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_visualization_layout: NULL argument");
  if ((dim != 2 && dim != 3) || (dim == 3 && axisymmetric))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_visualization_layout: dim 2 (planar or axisymmetric) or 3");
  return guarded([&] { vis_layout(*physics, dim, axisymmetric, out); });
}

int tpsrhs_visualization_fields(tpsrhs_handle h, const double *x, double *out) {
  if (!h || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_visualization_fields: NULL argument");
  return guarded([&] {
    tpsrhs_vis_layout l;
    vis_layout(h->phys, h->dim, h->nvel > h->dim ? 1 : 0, &l);  // refuses dry air and the table gas
    if (h->mixlen.distance)
      throw Unsupported("visualization fields: a mixing length is set; the reference would evaluate MixingLengthTransport "
                        "with the wall distance and the radius here, which is not built");
    if (h->ext.num_reactions > 0)
      throw Unsupported("visualization fields: the operator has reactions with an external rate coefficient; the progress-rate "
                        "rows index the full reaction list, which no kernel sees (DESIGN.md section 1)");
    load_plasma_vis_family(h, "visualization fields");
    HIP_CHECK(hipSetDevice(h->device));
    h->launch(h, x, nullptr, true);  // rhsOperator->updateGradients(*U, false): Up and gradUp of x
    const VisRows rows = {l.Xsp, l.Ysp, l.nsp_, l.FluxTrns, l.diffVel, l.SrcTrns, l.SpeciesTrns, l.rxn};
    h->vis_fields(h, rows, x, out);
  });
}

}  // extern "C"
