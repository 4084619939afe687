// libtpsrhs.so -- implementation of include/tpsrhs.h for gfx950 (MI355X).
//
// Host side: builds the face topology and the 1-D operator tables, keeps every field resident in
// HBM, and enqueues the three sweeps of kernels.hpp on one HIP stream per operator.  There is no
// CPU fallback: without a HIP device tpsrhs_create returns TPSRHS_ERR_NO_DEVICE.
#include "operator.hpp"
#include "element_geometry.hpp"
#include "integrals.hpp"
#include "locate_device.hpp"
#include "operator_plan.hpp"
#include "physics_dryair.hpp"
#include "physics_dryair_axisym.hpp"
#include "physics_plasma.hpp"
#include "plasma_params_host.hpp"
#include "point_locate.hpp"
#include "record_log.hpp"
#include "sampling.hpp"
#include "statistics.hpp"
#include "time_integrators.hpp"
#include "wall_distance.hpp"
#include "wall_faces.hpp"

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
void pick_dryair_les(tpsrhs_operator *op);

static thread_local std::string g_last_error;

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

// LinearTable::LinearTable (src/table.cpp:39-50): interval coefficients (plasma_params_host.hpp), uploaded with the abscissae
TableDev upload_table(tpsrhs_operator *op, const tpsrhs_table &t) {
  std::vector<double> buf;
  TableDev td = table_coeffs(t, buf);
  op->d_extra.emplace_back(DevBuf<double>(buf));
  double *d = static_cast<double *>(op->d_extra.back().get());
  td.x = d;
  td.a = d + td.n;
  td.b = d + 2 * td.n;
  return td;
}

// the polynomial table of the Coulomb fits (coulomb_table.hpp), filled once per process from the literals of the closure
const std::vector<double> &coulomb_table_host() {
  static const std::vector<double> table = [] {
    std::vector<double> t(coulomb::SIZE);
    coll::coulomb_table_fill(t.data());
    return t;
  }();
  return table;
}

// the parameter block of the plasma kernels (plasma_params_host.hpp) into the operator, the chemistry block to the device
template <int NSP>
void fill_plasma_params(tpsrhs_operator *op, const tpsrhs_disc *disc, const tpsrhs_physics *phys, int num_bcs,
                        const tpsrhs_bc *bcs) {
  static_assert(sizeof(PlasmaParams<NSP>) <= sizeof(op->params), "parameter block too large");
  PlasmaParams<NSP> &p = *new (op->params) PlasmaParams<NSP>;
  std::unique_ptr<ChemDev> c(new ChemDev);
  try {
    tpsrhs::fill_plasma_params<NSP>(p, *c, disc, phys, num_bcs, bcs, [op](const tpsrhs_table &t) { return upload_table(op, t); });
  } catch (const UnsupportedConfig &e) {  // (its header is also built alone, on the host, by tests/host_physics: it keeps its own type)
    throw Unsupported(e.what());
  }
  op->d_chem = DevBuf<ChemDev>(1);
  p.chem = static_cast<ChemDev *>(op->d_chem.get());
  HIP_CHECK(hipMemcpy(op->d_chem.get(), c.get(), sizeof(ChemDev), hipMemcpyHostToDevice));
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
  lp->tab_e = upload_table(op, in.energy_table);
  lp->tab_R = upload_table(op, in.gas_constant_table);
  lp->tab_c = upload_table(op, in.sound_speed_table);
  tpsrhs_table rev = in.energy_table;  // "Construct e -> T table from T -> e", src/M2ulPhyS.cpp:193-200
  rev.x_data = in.energy_table.f_data;
  rev.f_data = in.energy_table.x_data;
  lp->tab_T = upload_table(op, rev);
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
  lp->tab_mu = upload_table(op, in.viscosity_table);
  lp->tab_k = upload_table(op, in.conductivity_table);
  lp->tab_sigma = upload_table(op, in.electric_conductivity_table);
  lp->radiation = phys->radiation.model;
  if (lp->radiation == TPSRHS_NET_EMISSION) lp->tab_nec = upload_table(op, phys->radiation.nec_table);
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
  static_assert(sizeof(LteParams) <= sizeof(op->params), "parameter block");
  LteParams *lp = pl.lte ? new (op->params) LteParams : nullptr;
  if (lp) std::memset(static_cast<void *>(lp), 0, sizeof(LteParams));
  DryAirParams &d = lp ? *static_cast<DryAirParams *>(lp) : *new (op->params) DryAirParams;
  if (!lp) std::memset(&d, 0, sizeof(d));
  if (lp) upload_lte_tables(op, lp, phys);
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
    throw std::runtime_error("halo: a partitioned mesh with non-reflecting patches needs runtime.reduce");
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

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    struct NoDevice : std::runtime_error {
      NoDevice() : std::runtime_error("no HIP device visible; tpsrhs has no CPU path") {}
    };
    throw NoDevice();
  }
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

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

template <class F>
int guarded(F &&f) {
  try {
    f();
    return TPSRHS_OK;
  } catch (const Unsupported &e) {
    return fail(TPSRHS_ERR_UNSUPPORTED, e.what());
  } catch (const DeviceError &e) {
    return fail(TPSRHS_ERR_DEVICE, e.what());
  } catch (const std::invalid_argument &e) {
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, e.what());
  } catch (const std::runtime_error &e) {
    const std::string w = e.what();
    if (w.find("no HIP device") != std::string::npos) return fail(TPSRHS_ERR_NO_DEVICE, w);
    if (w.find("halo") != std::string::npos) return fail(TPSRHS_ERR_HALO, w);
    return fail(TPSRHS_ERR_MESH, w);
  } catch (const std::exception &e) {
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, e.what());
  }
}

// Running statistics (statistics.hpp): at the end of this file
void stats_release(tpsrhs_operator *h);
void stats_sample(tpsrhs_operator *h, const double *x);
// Probe records (sampling.hpp): at the end of this file
void sampling_release(tpsrhs_operator *h);
void transfer_release(tpsrhs_operator *h);
void probe_record(tpsrhs_operator *h, const double *x);
// Monitor records (integrals.hpp): at the end of this file
void integrals_release(tpsrhs_operator *h);
void monitor_record(tpsrhs_operator *h, const double *x);
// What the time loop does between two steps, and whether any of it falls after the first of the next two: everything that
// reads x between steps goes through these two, so that the loop itself knows nothing about statistics, probes or the
// monitor.  Each observer has one StepCadence (record_log.hpp; interval 0: off), which answers both questions.
inline void after_step(tpsrhs_operator *h, const double *x) {
  if (h->stats && h->stats->cadence.tick()) stats_sample(h, x);
  if (h->sampling && h->sampling->probe.cadence.tick()) probe_record(h, x);
  if (h->integrals && h->integrals->monitor.cadence.tick()) monitor_record(h, x);
}
inline bool work_due_after_next(const tpsrhs_operator *h) {
  return (h->stats && h->stats->cadence.due_after_next()) || (h->sampling && h->sampling->probe.cadence.due_after_next()) ||
         (h->integrals && h->integrals->monitor.cadence.due_after_next());
}

// f(std::integral_constant<int, DIM>, std::integral_constant<int, P>) for the operator's dim and order: the (dim, order) pairs
// the post-processing kernels of this unit are built for, listed once
template <int N>
using int_c = std::integral_constant<int, N>;
template <class F>
void with_dim_order(const tpsrhs_operator *h, const char *who, F &&f) {
  switch (h->dim * 10 + h->order) {
    case 21: f(int_c<2>(), int_c<1>()); break;
    case 22: f(int_c<2>(), int_c<2>()); break;
    case 23: f(int_c<2>(), int_c<3>()); break;
    case 24: f(int_c<2>(), int_c<4>()); break;
    case 25: f(int_c<2>(), int_c<5>()); break;
    case 31: f(int_c<3>(), int_c<1>()); break;
    case 32: f(int_c<3>(), int_c<2>()); break;
    case 33: f(int_c<3>(), int_c<3>()); break;
    case 34: f(int_c<3>(), int_c<4>()); break;
    case 35: f(int_c<3>(), int_c<5>()); break;
    default: throw Unsupported(std::string(who) + ": dim 2 or 3 and polynomial orders 1..5 are built");
  }
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
  stats_release(h);
  transfer_release(h);
  sampling_release(h);
  integrals_release(h);
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

// ---- the device time loop ------------------------------------------------------------------------------------------------
// Its state is tpsrhs_operator::loop; the rules are in trace_chain.hpp.  The functions stay in this order, and rk_stages
// after every other launch of this unit: the compiler numbers a unit's kernels by their first launch in the source, and
// tools/device_asm_diff.py compares the local labels that carry that number.
namespace {
// The stage vectors in loop.d_rk (3 n doubles, with loop.d_nan allocated at the first step): k | y | z, or k | y with y on
// an even offset, so that an odd n keeps the 16-byte accesses (y then ends at or before 2 n + 1 <= 3 n).
struct StageScratch {
  double *k, *y, *z;
};
StageScratch stage_scratch(tpsrhs_operator *h, int64_t n, bool even_offsets) {
  tpsrhs_operator::TimeLoop &lp = h->loop;
  if (!lp.d_rk) {
    lp.d_rk = DevBuf<double>(3 * n);
    lp.d_nan = DevBuf<unsigned long long>(1);
    HIP_CHECK(hipMemsetAsync(lp.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
  }
  double *k = lp.d_rk.get();
  if (even_offsets) return {k, k + ((n + 1) & ~static_cast<int64_t>(1)), nullptr};
  return {k, k + n, k + 2 * n};
}
// {dt, time, max speed} of the loop in device memory; the probe and monitor records copy the time from there
double *loop_ctl(tpsrhs_operator *h) {
  if (!h->loop.d_ctl) h->loop.d_ctl = DevBuf<double>(3);
  return h->loop.d_ctl.get();
}

// the four stages of MFEM's RK4Solver::Step around Mult; dt by value or from device memory (dt_dev)
void rk4_stages(tpsrhs_operator *h, double *x, double dt, const double *dt_dev) {
  const int64_t n = static_cast<int64_t>(h->neq) * h->ndofs;
  const StageScratch sc = stage_scratch(h, n, false);
  double *k = sc.k, *y = sc.y, *z = sc.z;
  TraceChain &chain = h->loop.chain;
  chain.begin_step();
  ScopeExit step([&](bool) { chain.end_step(); });
  const int sp_first = h->loop.sp_first, sp_last = h->loop.sp_last;
  const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 8192));
  if (!h->forcing_active) {
    // The stage combinations in k_flux's epilogue (RkDev, kernels.hpp): k never goes to memory, the accumulator of
    // RK4Solver::Step is recovered from the stage states at the end.  (The optional forcing terms add to the residual in
    // a pass of their own after k_flux: with them the separate stage kernel below stays.)
    double *y2 = k, *y3 = y, *y4 = z;  // the three stage states
    const double *ins[4] = {x, y2, y3, y4};
    double *outs[4] = {y2, y3, y4, x};
    for (int stage = 1; stage <= 4; stage++) {
      RkDev r = {};
      r.mode = stage;
      r.sp_first = sp_first;
      r.sp_last = sp_last;
      r.dt_host = dt;
      r.dt_dev = dt_dev;
      r.x0 = x;
      r.y2 = y2;
      r.y3 = y3;
      r.y4 = y4;
      r.out = outs[stage - 1];
      r.nan_count = h->loop.d_nan.get();
      h->rk = r;  // in force for this launch only
      ScopeExit launched([&](bool failed) {
        h->rk = RkDev{};
        if (failed) chain.abandon();
      });
      h->launch(h, ins[stage - 1], outs[stage - 1], false);
    }
    return;
  }
  const double *in = x;
  for (int stage = 1; stage <= 4; stage++) {
    h->launch(h, in, k, false);  // k_s = f(stage input); SetTime is a no-op for this operator
    hipLaunchKernelGGL(k_rk4_stage<256>, dim3(grid), dim3(256), 0, h->stream, stage, n, h->ndofs, sp_first, sp_last, dt,
                       dt_dev, x, k, y, z, h->loop.d_nan.get());
    HIP_CHECK(hipGetLastError());
    in = y;
  }
}

// Forward Euler, RK2(a = 1) and RK3-SSP: at the end of this file
void rk_stages(tpsrhs_operator *h, int integrator, double *x, double dt, const double *dt_dev);

// TPSRHS_OK for the integrators that are built; the status of the others, before any device work
int check_integrator(int integrator, const char *who) {
  switch (integrator) {
    case TPSRHS_FORWARD_EULER:
    case TPSRHS_RK2:
    case TPSRHS_RK3_SSP:
    case TPSRHS_RK4: return TPSRHS_OK;
    case TPSRHS_RK6:
      return fail(TPSRHS_ERR_UNSUPPORTED, std::string(who) + ": the RK6 integrator (MFEM's eight-stage Verner scheme) is not built; "
                                              "forwardEuler, rk2, rk3 and rk4 are");
    default:
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown integrator " + std::to_string(integrator) +
                                                   " (the reference's timeIntegratorType: 1, 2, 3, 4 or 6)");
  }
}

void step_stages(tpsrhs_operator *h, int integrator, double *x, double dt, const double *dt_dev) {
  if (integrator == TPSRHS_RK4)
    rk4_stages(h, x, dt, dt_dev);
  else
    rk_stages(h, integrator, x, dt, dt_dev);
}

int step_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double dt, double *max_char_speed,
              int64_t *nan_count);
int advance_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double *dt, int num_steps,
                 int constant_dt, double cfl, double hmin, int64_t *nan_count);
}  // namespace

int tpsrhs_rk4_step(tpsrhs_handle h, double *x, double *time, double dt, double *max_char_speed, int64_t *nan_count) {
  return step_with(h, TPSRHS_RK4, "tpsrhs_rk4_step", x, time, dt, max_char_speed, nan_count);
}

int tpsrhs_step(tpsrhs_handle h, int integrator, double *x, double *time, double dt, double *max_char_speed,
                int64_t *nan_count) {
  return step_with(h, integrator, "tpsrhs_step", x, time, dt, max_char_speed, nan_count);
}

int tpsrhs_advance(tpsrhs_handle h, double *x, double *time, double *dt, int num_steps, int constant_dt, double cfl,
                   double hmin, int64_t *nan_count) {
  return advance_with(h, TPSRHS_RK4, "tpsrhs_advance", x, time, dt, num_steps, constant_dt, cfl, hmin, nan_count);
}

int tpsrhs_advance_with(tpsrhs_handle h, int integrator, double *x, double *time, double *dt, int num_steps,
                        int constant_dt, double cfl, double hmin, int64_t *nan_count) {
  return advance_with(h, integrator, "tpsrhs_advance_with", x, time, dt, num_steps, constant_dt, cfl, hmin, nan_count);
}

}  // extern "C"

namespace {
int step_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double dt, double *max_char_speed,
              int64_t *nan_count) {
  if (!h || !x || !time) return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (const int st = check_integrator(integrator, who)) return st;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    h->nr_dt = dt;  // the boundary conditions see M2ulPhyS::dt (src/BoundaryCondition.hpp:54)
    if (h->loop.d_nan) HIP_CHECK(hipMemsetAsync(h->loop.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
    step_stages(h, integrator, x, dt, nullptr);
    *time += dt;
    if (max_char_speed || nan_count) {
      hipLaunchKernelGGL(k_reduce_max<1024>, dim3(1), dim3(1024), 0, h->stream, h->flux_grid, h->d_block_speed.get(), h->d_speed.get());
      HIP_CHECK(hipGetLastError());
      double speed = 0.0;
      unsigned long long bad = 0;
      HIP_CHECK(hipMemcpyAsync(&speed, h->d_speed.get(), sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipMemcpyAsync(&bad, h->loop.d_nan.get(), sizeof(bad), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipStreamSynchronize(h->stream));
      if (max_char_speed) *max_char_speed = speed;
      if (nan_count) *nan_count = static_cast<int64_t>(bad);
    }
  });
}

// The stage sequence (step_stages) is all that depends on the integrator: the end of the step, the MIN reduce, the graph,
// the error paths and the read-back are shared.
int advance_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double *dt, int num_steps,
                 int constant_dt, double cfl, double hmin, int64_t *nan_count) {
  if (!h || !x || !time || !dt) return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (const int st = check_integrator(integrator, who)) return st;
  if (num_steps < 0 || !(*dt > 0.0) || (!constant_dt && !(cfl > 0.0 && hmin > 0.0)))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": needs num_steps >= 0, dt > 0 and (constant dt or cfl, hmin > 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (!constant_dt && h->topo.num_shared > 0 && !h->reduce)
      throw std::runtime_error("halo: a variable time step on a partitioned mesh needs runtime.reduce");
    double *const d_ctl = loop_ctl(h);
    const double ctl0[3] = {*dt, *time, 0.0};
    HIP_CHECK(hipMemcpyAsync(d_ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));  // ctl0 lives on this stack frame
    if (h->loop.d_nan) HIP_CHECK(hipMemsetAsync(h->loop.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
    const double coef = cfl * hmin / static_cast<double>(h->dim);
    auto one_step = [&] {
      step_stages(h, integrator, x, 0.0, d_ctl);
      hipLaunchKernelGGL(k_step_end<1024>, dim3(1), dim3(1024), 0, h->stream, h->flux_grid, h->d_block_speed.get(), d_ctl,
                         constant_dt ? 1 : 0, coef);
      HIP_CHECK(hipGetLastError());
      if (!constant_dt && h->reduce && h->topo.num_shared > 0) {  // MPI_Allreduce(MIN) of src/M2ulPhyS.cpp:2015
        if (h->reduce(h->reduce_ctx, d_ctl, 1, TPSRHS_REDUCE_MIN, h->stream) != 0)
          throw std::runtime_error("halo: reduce callback failed");
      }
    };
    // On one rank a step is a fixed sequence of launches (~17 for RK4) whose arguments do not change from step to step (dt
    // and the time are in device memory; the two boundary-state buffers swap four times per step): captured once
    // into a hipGraph and replayed -- the launch overhead matters on small meshes.  Needs a capturable stream (not
    // the NULL stream), no host callbacks in the step (partitioned meshes keep the plain loop), no timing events.
    const char *genv = std::getenv("TPSRHS_GRAPH");
    const bool use_graph = h->stream != nullptr && h->topo.num_shared == 0 && !h->timing && num_steps >= 3 &&
                           !(genv && genv[0] == '0');
    const int per_graph = steps_per_graph(integrator, h->n_nr_faces > 0);
    {
      // the session: the boundary conditions read dt from device memory, the steps are chained; put back however it ends
      h->nr_dt_dev = d_ctl;
      h->loop.chain.begin_advance(integrator == TPSRHS_RK4 && !h->forcing_active);
      ScopeExit session([&](bool) {
        h->nr_dt_dev = nullptr;
        h->loop.chain.end_advance();
      });
      // Running statistics and probe records: the host issues every step anyway and knows the iteration number, so it
      // enqueues the sample or the record between two steps -- never inside the captured graph, whose key knows about neither.
      int step = 0;
      if (use_graph) {
        one_step();  // first step outside the graph: allocations, initial boundary state, its own k_traces sweep
        after_step(h, x);
        step = 1;
        StepKey key;
        key.x = x;
        key.constant_dt = constant_dt ? 1 : 0;
        key.bstate_cur = h->bstate_cur;
        key.epoch = h->loop.config_epoch;
        key.integrator = integrator;
        key.coef = coef;
        h->loop.graph.ensure(key, h->stream, [&] {
          for (int i = 0; i < per_graph; i++) one_step();
        });
        for (; step + per_graph <= num_steps; step += per_graph) {
          // a sample or a record between the two steps of one graph: the pair runs as two plain steps (bit-equal to the
          // replay, as the odd remainder below is), which leave the boundary-state buffers as the graph does
          const bool split = per_graph == 2 && work_due_after_next(h);
          for (int i = 0; i < per_graph; i++) {
            if (split)
              one_step();
            else if (i == 0)
              h->loop.graph.launch(h->stream);
            after_step(h, x);
          }
        }
      }
      for (; step < num_steps; step++) {
        one_step();
        after_step(h, x);
      }
    }
    double ctl[3] = {0, 0, 0};
    unsigned long long bad = 0;
    HIP_CHECK(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, h->stream));
    if (h->loop.d_nan) HIP_CHECK(hipMemcpyAsync(&bad, h->loop.d_nan.get(), sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    *dt = ctl[0];
    *time = ctl[1];
    h->nr_dt = ctl[0];
    if (nan_count) *nan_count = static_cast<int64_t>(bad);
  });
}
}  // namespace

extern "C" {

int tpsrhs_set_dt(tpsrhs_handle h, double dt) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_dt: NULL handle");
  h->nr_dt = dt;
  return TPSRHS_OK;
}

namespace {
void upload_forcing(tpsrhs_operator *h) {
  const ForcingDev &f = h->forcing;
  h->forcing_active = f.has_pg || f.nheat > 0 || f.nsponge > 0 || f.nps > 0 || f.joule != nullptr;
  if (!h->forcing_active) return;
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
    const bool prev_active = h->forcing_active;
    h->forcing = f;
    {
      ScopeExit rollback([&](bool failed) {
        if (failed) {
          h->forcing = prev;
          h->forcing_active = prev_active;
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

namespace {
__global__ void k_table_eval(TableDev t, int64_t n, const double *__restrict__ x, double *__restrict__ f) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) f[i] = table_eval(t, x[i]);
}
}  // namespace

namespace {
__global__ void k_math_eval(int fn, int64_t n, const double *__restrict__ x, double *__restrict__ y) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  switch (fn) {
    case 0: r = fexp(v); break;
    case 1: r = fexp<false>(v); break;
    case 2: r = flog(v); break;
    case 3: r = flog_pos(v); break;
    case 4: r = fast_rcp(v); break;
    case 5: r = fast_sqrt(v); break;
    default: r = fast_rsqrt(v); break;
  }
  y[i] = r;
}
}  // namespace

int tpsrhs_math_eval(int function, int64_t n, const double *x, double *y) {
  if (function < 0 || function > 6 || n < 0 || !x || !y) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "math_eval");
  return guarded([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device visible");
    if (n > 0) {
      hipLaunchKernelGGL(k_math_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, function, n, x, y);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}

namespace {
// route 0: cfit_n; 1: the table with two wave-uniform rounds, then lane by lane; 2: lane by lane only.  1 / Tp^2 = 1.
__global__ void k_coulomb_eval(int route, const double *tab, int64_t n, const double *__restrict__ x, double *__restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  coll::Arg a;
  a.ln = x[i];
  a.inv2 = 1.0;
  double g[8];
  if (route == 0 || !coulomb::in_range(a.ln)) {
    coll::cfit_tab<8>(nullptr, a, g);
  } else if (route == 1) {
    coll::ctab_eval<8, 2>(tab, a.ln, true, g);
  } else {
    coll::ctab_eval<8, 0>(tab, a.ln, true, g);
  }
#pragma unroll
  for (int f = 0; f < 8; f++) out[f * n + i] = g[f];
}
}  // namespace

// route 3, the LDS window of a wave: coulomb_probe.hip (a unit of its own -- a kernel added to this one renumbers the labels of
// every kernel the compiler emits after it, and the device code of this unit is compared from commit to commit)
// (C++ linkage: this declaration stands inside an extern "C" block)
extern "C++" void coulomb_probe_window(const double *tab, int64_t n, const double *x, double *out);

int tpsrhs_coulomb_eval(int route, int64_t n, const double *x, double *out) {
  if (route < 0 || route > 3 || n < 0 || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "coulomb_eval");
  return guarded([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device visible");
    DevBuf<double> tab(coulomb_table_host());  // its own table, from the same fill as an operator's
    if (n > 0 && route == 3) {
      coulomb_probe_window(tab.get(), n, x, out);
      HIP_CHECK(hipGetLastError());
    } else if (n > 0) {
      hipLaunchKernelGGL(k_coulomb_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, route, tab.get(), n, x, out);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int tpsrhs_table_eval(const tpsrhs_table *table, int64_t n, const double *x, double *f) {
  if (!table || n < 0 || !x || !f) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "table_eval");
  return guarded([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device visible");
    tpsrhs_operator tmp;  // owns the device copy of the table for the duration of the call
    (void)hipGetDevice(&tmp.device);
    const TableDev td = upload_table(&tmp, *table);
    if (n > 0) {
      hipLaunchKernelGGL(k_table_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, td, n, x, f);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
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
const char *tpsrhs_last_error(void) { return g_last_error.c_str(); }
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

namespace {
// Forward Euler, RK2(a = 1) and RK3-SSP (time_integrators.hpp): the plain Mult (h->rk stays RkDev{}: k_flux writes the
// residual, nothing enters the trace chain) and one k_rk_stage pass per stage.  (Fusing these combinations into k_flux's
// epilogue, as RK4 has, is left out on purpose: DESIGN.md section 9.)  Here, after every other launch of this unit: see
// the head of the time loop's section.
template <int OP>
void rk_stage(tpsrhs_operator *h, int64_t n, int64_t clamp_lo, int64_t clamp_hi, double dt, const double *dt_dev, double *x,
              const double *k, double *y) {
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int64_t items = vec ? (n + 1) / 2 : n;
  const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 8192));  // the grid cap of k_rk4_stage
  if (vec)
    hipLaunchKernelGGL((k_rk_stage<OP, true, 256>), dim3(grid), dim3(256), 0, h->stream, n, clamp_lo, clamp_hi, dt, dt_dev, x, k, y,
                       h->loop.d_nan.get());
  else
    hipLaunchKernelGGL((k_rk_stage<OP, false, 256>), dim3(grid), dim3(256), 0, h->stream, n, clamp_lo, clamp_hi, dt, dt_dev, x, k, y,
                       h->loop.d_nan.get());
  HIP_CHECK(hipGetLastError());
}

void rk_stages(tpsrhs_operator *h, int integrator, double *x, double dt, const double *dt_dev) {
  const int64_t n = static_cast<int64_t>(h->neq) * h->ndofs;
  const StageScratch sc = stage_scratch(h, n, true);
  double *k = sc.k, *y = sc.y;
  h->loop.chain.begin_step();  // every Mult of these schemes runs its own k_traces sweep
  ScopeExit step([h](bool) { h->loop.chain.end_step(); });
  // Check_Undershoot's rows, contiguous in [neq][ndofs]
  const int64_t lo = h->loop.sp_first * h->ndofs, hi = h->loop.sp_last * h->ndofs;
  h->launch(h, x, k, false);  // k = f(x); SetTime is a no-op for this operator
  if (integrator == TPSRHS_FORWARD_EULER) {
    rk_stage<RK_EULER>(h, n, lo, hi, dt, dt_dev, x, k, y);
  } else if (integrator == TPSRHS_RK2) {
    rk_stage<RK2_STAGE1>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK2_STAGE2>(h, n, lo, hi, dt, dt_dev, x, k, y);
  } else {
    rk_stage<RK3_STAGE1>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK3_STAGE2>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK3_STAGE3>(h, n, lo, hi, dt, dt_dev, x, k, y);
  }
}
}  // namespace

// ---- running mean and velocity covariances (statistics.hpp) ----------------------------------------------------------------
// After every other launch of this unit, as the integrators above.
namespace {
void stats_release(tpsrhs_operator *h) {
  tpsrhs_stats_state *st = h->stats;
  if (!st) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a sample may still be running
  delete st;
  h->stats = nullptr;
}

template <int NVEL, bool VARI>
void launch_stats_sample(tpsrhs_operator *h) {
  tpsrhs_stats_state *st = h->stats;
  const int64_t n = h->ndofs;
  const double *prim = st->d_scratch.get(), *p = prim + h->neq * n;
  double *mean = st->d_mean.get(), *vari = st->d_vari.get();
  const uintptr_t bits = reinterpret_cast<uintptr_t>(prim) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(vari);
  const bool vec = (n & 1) == 0 && (bits & 15) == 0;  // then every row of every array is 16-byte aligned, p included
  const int64_t items = vec ? n / 2 : n;
  const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 8192));  // the grid cap of k_rk_stage
  if (grid == 0) return;
  if (vec)
    hipLaunchKernelGGL((k_stats_sample<NVEL, VARI, true, 256>), dim3(grid), dim3(256), 0, h->stream, h->neq, n, st->ns_mean,
                       st->ns_vari, prim, p, mean, vari);
  else
    hipLaunchKernelGGL((k_stats_sample<NVEL, VARI, false, 256>), dim3(grid), dim3(256), 0, h->stream, h->neq, n, st->ns_mean,
                       st->ns_vari, prim, p, mean, vari);
  HIP_CHECK(hipGetLastError());
}

// One sample of the device vector x, stream-ordered: the primitives and the pressure from the gas model's own point-wise
// kernel (tpsrhs_eval_pointwise quantities 0 and 1: no physics here), then the update.  The counters are host integers.
void stats_sample(tpsrhs_operator *h, const double *x) {
  tpsrhs_stats_state *st = h->stats;
  const int64_t n = h->ndofs;
  h->point_eval(h, 0, n, x, st->d_scratch.get());
  h->point_eval(h, 1, n, x, st->d_scratch.get() + h->neq * n);
  const bool vari = st->nvar > 0;
  if (h->nvel == 3)
    vari ? launch_stats_sample<3, true>(h) : launch_stats_sample<3, false>(h);
  else
    vari ? launch_stats_sample<2, true>(h) : launch_stats_sample<2, false>(h);
  st->ns_mean++;
  st->ns_vari++;
}

// the statistics of h, or NULL with the error text set
tpsrhs_stats_state *stats_of(tpsrhs_handle h, const char *who) {
  if (!h) {
    fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL handle");
    return nullptr;
  }
  if (!h->stats) fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": statistics are not configured (tpsrhs_stats_configure)");
  return h->stats;
}
}  // namespace

extern "C" {

int tpsrhs_stats_configure(tpsrhs_handle h, int64_t sample_interval, int64_t start_iter, int compute_variances) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_configure: NULL handle");
  if (sample_interval < 0 || start_iter < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_configure: needs sample_interval >= 0 (0: off) and start_iter >= 0");
  if (sample_interval > 0 && h->nvel != 2 && h->nvel != 3)
    return fail(TPSRHS_ERR_UNSUPPORTED, "tpsrhs_stats_configure: two or three velocity components");
  return guarded([&] {
    stats_release(h);
    if (sample_interval == 0) return;
    HIP_CHECK(hipSetDevice(h->device));
    std::unique_ptr<tpsrhs_stats_state> st(new tpsrhs_stats_state());
    st->cadence.interval = sample_interval;
    st->cadence.start = start_iter;
    st->nvar = compute_variances ? h->nvel * (h->nvel + 1) / 2 : 0;
    const int64_t n = h->ndofs;
    st->d_mean = DevBuf<double>(h->neq * n);
    if (st->nvar) st->d_vari = DevBuf<double>(st->nvar * n);
    st->d_scratch = DevBuf<double>((h->neq + 1) * n);
    HIP_CHECK(hipMemsetAsync(st->d_mean.get(), 0, sizeof(double) * h->neq * n, h->stream));
    if (st->nvar) HIP_CHECK(hipMemsetAsync(st->d_vari.get(), 0, sizeof(double) * st->nvar * n, h->stream));
    h->stats = st.release();  // complete: a call that throws above leaves the statistics off
  });
}

int tpsrhs_stats_set_iter(tpsrhs_handle h, int64_t iter) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_set_iter");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (iter < 0) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set_iter: needs iter >= 0");
  st->cadence.count = iter;
  return TPSRHS_OK;
}

int tpsrhs_stats_add_sample(tpsrhs_handle h, const double *x) {
  if (!stats_of(h, "tpsrhs_stats_add_sample")) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (!x) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_add_sample: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    stats_sample(h, x);
  });
}

int tpsrhs_stats_get(tpsrhs_handle h, double *mean_out, double *vari_out, int *ns_mean, int *ns_vari, int64_t *iter) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_get");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (vari_out && !st->nvar)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_get: the covariances are not computed (compute_variances = 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int64_t n = h->ndofs;
    if (mean_out) HIP_CHECK(hipMemcpyAsync(mean_out, st->d_mean.get(), sizeof(double) * h->neq * n, hipMemcpyDeviceToDevice, h->stream));
    if (vari_out) HIP_CHECK(hipMemcpyAsync(vari_out, st->d_vari.get(), sizeof(double) * st->nvar * n, hipMemcpyDeviceToDevice, h->stream));
    if (ns_mean) *ns_mean = st->ns_mean;
    if (ns_vari) *ns_vari = st->ns_vari;
    if (iter) *iter = st->cadence.count;
  });
}

int tpsrhs_stats_set(tpsrhs_handle h, const double *mean, const double *vari, int ns_mean, int ns_vari) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_set");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (ns_mean < 0 || ns_vari < 0 || (ns_mean > 0 && !mean))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set: needs counters >= 0 and the mean field of ns_mean > 0 samples");
  if (vari && ns_vari > 0 && !st->nvar)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set: the covariances are not computed (compute_variances = 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int64_t n = h->ndofs;
    const bool keep_vari = vari && ns_vari > 0;  // else restartRMS: the covariances start again
    if (ns_mean > 0)
      HIP_CHECK(hipMemcpyAsync(st->d_mean.get(), mean, sizeof(double) * h->neq * n, hipMemcpyDeviceToDevice, h->stream));
    else
      HIP_CHECK(hipMemsetAsync(st->d_mean.get(), 0, sizeof(double) * h->neq * n, h->stream));
    if (st->nvar) {
      if (keep_vari)
        HIP_CHECK(hipMemcpyAsync(st->d_vari.get(), vari, sizeof(double) * st->nvar * n, hipMemcpyDeviceToDevice, h->stream));
      else
        HIP_CHECK(hipMemsetAsync(st->d_vari.get(), 0, sizeof(double) * st->nvar * n, h->stream));
    }
    st->ns_mean = ns_mean;
    st->ns_vari = keep_vari ? ns_vari : 0;
  });
}

int tpsrhs_stats_num_variances(tpsrhs_handle h, int *num_variances) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_num_variances");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (!num_variances) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_num_variances: NULL argument");
  *num_variances = st->nvar;
  return TPSRHS_OK;
}

}  // extern "C"

// ---- point sampling and probe records (sampling.hpp, point_locate.hpp) --------------------------------------------------------
// After every other launch of this unit, as the integrators and the statistics above.
namespace {
// What reading the probe records and reading the monitor records share.  The first n rows of one column of a log (`width`
// doubles a row) to the host, on the operator's stream ...
void fetch_rows(tpsrhs_operator *h, double *dst, const DevBuf<double> &col, int64_t n, int64_t width) {
  if (dst && n * width) HIP_CHECK(hipMemcpyAsync(dst, col.get(), sizeof(double) * n * width, hipMemcpyDeviceToHost, h->stream));
}
// ... and, once the stream has been synchronised, the host half: the counters, the step of every record, the optional restart
void read_index(RecordIndex &ix, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, int reset) {
  if (nrecords) *nrecords = ix.nrecords;
  if (ndropped) *ndropped = ix.ndropped;
  if (iters_out && ix.nrecords) std::memcpy(iters_out, ix.iters.data(), sizeof(int64_t) * ix.nrecords);
  if (reset) ix.reset();  // the buffer starts again; the step counter goes on
}

void probe_off(tpsrhs_operator *h) {
  tpsrhs_sampling_state *ss = h->sampling;
  if (!ss || !ss->probe.sampler) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a record may still be running
  ss->probe = tpsrhs_probe_log();
}

void sampling_release(tpsrhs_operator *h) {
  tpsrhs_sampling_state *ss = h->sampling;
  if (!ss) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a sample may still be running
  delete ss;
  h->sampling = nullptr;
}

// The sources of tpsrhs_transfer that hold a cached sampler: the destruction of ANY operator looks here for samplers at
// its nodes (the cache is keyed by the address of dst, which the next tpsrhs_create may hand out again).
std::mutex g_transfer_mu;
std::vector<tpsrhs_operator *> g_transfer_sources;

void sampler_remove(tpsrhs_operator *h, tpsrhs_sampler *s);

// h is being destroyed: forget it as a source (sampling_release frees its samplers) and drop every sampler at its nodes
void transfer_release(tpsrhs_operator *h) {
  std::lock_guard<std::mutex> lock(g_transfer_mu);
  auto &src = g_transfer_sources;
  src.erase(std::remove(src.begin(), src.end(), h), src.end());
  for (tpsrhs_operator *o : src) {
    auto &tr = o->sampling->transfers;  // exists: o holds a cached sampler
    for (size_t k = tr.size(); k-- > 0;)
      if (tr[k].dst == h) {
        sampler_remove(o, tr[k].sampler);
        tr.erase(tr.begin() + static_cast<std::ptrdiff_t>(k));
      }
  }
}

template <int DIM, int P>
void launch_sample(tpsrhs_operator *h, const tpsrhs_sampler *s, const SampleNodes &nodes, int nrows, const double *field,
                   double *out) {
  constexpr int BLOCK = 64;  // one wave: 64 probes are one block, a plane of 65 536 points is 1024 blocks over the 256 CUs
  const int64_t grid = (s->npts + BLOCK - 1) / BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_sample: more than 2^37 points");
  hipLaunchKernelGGL((k_sample<DIM, P, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, s->npts, nrows,
                     h->ndofs, nodes, s->d_elem.get(), s->d_ref.get(), s->d_perm.get(), s->fill, field, out);
  HIP_CHECK(hipGetLastError());
}

// out[nrows][npts] = field[nrows][NDofs] at the points of s, on the operator's stream
void sample_field(tpsrhs_operator *h, const tpsrhs_sampler *s, int nrows, const double *field, double *out) {
  SampleNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // the nodes of the operator's basis, as make_tables places them
  with_dim_order(h, "tpsrhs_sample", [&](auto dim, auto p) {
    launch_sample<decltype(dim)::value, decltype(p)::value>(h, s, nodes, nrows, field, out);
  });
}

// One probe record of the device vector x, stream-ordered, or one more dropped record when the buffer is full.
void probe_record(tpsrhs_operator *h, const double *x) {
  tpsrhs_probe_log &log = h->sampling->probe;
  const int64_t r = log.index.claim(log.cadence.count);
  if (r < 0) return;
  const int64_t per = static_cast<int64_t>(h->neq) * log.sampler->npts;
  sample_field(h, log.sampler, h->neq, x, log.d_values.get() + r * per);
  HIP_CHECK(hipMemcpyAsync(log.d_times.get() + r, h->loop.d_ctl.get() + 1, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

// the position of s among the samplers of ss, or their end
auto sampler_find(tpsrhs_sampling_state *ss, const tpsrhs_sampler *s) {
  return std::find_if(ss->samplers.begin(), ss->samplers.end(), [s](const auto &u) { return u.get() == s; });
}

// s, a live sampler of h, leaves it
void sampler_remove(tpsrhs_operator *h, tpsrhs_sampler *s) {
  tpsrhs_sampling_state *ss = h->sampling;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a sample may still be running
  if (ss->probe.sampler == s) probe_off(h);
  ss->samplers.erase(sampler_find(ss, s));
}

// The host copies of a device-located sampler (elem, ref, nfound), fetched once; synchronises the stream.
void sampler_fetch(tpsrhs_sampler *s) {
  if (s->host_valid) return;
  tpsrhs_operator *h = s->owner;
  HIP_CHECK(hipSetDevice(h->device));
  unsigned long long nf = 0;
  s->elem.resize(static_cast<size_t>(s->npts));
  s->ref.resize(static_cast<size_t>(s->npts) * h->dim);
  HIP_CHECK(hipMemcpyAsync(&nf, s->d_nfound.get(), sizeof(nf), hipMemcpyDeviceToHost, h->stream));
  if (s->npts) {
    HIP_CHECK(hipMemcpyAsync(s->elem.data(), s->d_elem.get(), s->elem.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(s->ref.data(), s->d_ref.get(), s->ref.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_CHECK(hipStreamSynchronize(h->stream));
  s->nfound = static_cast<int64_t>(nf);
  s->host_valid = true;
}
// ... and the count alone (tpsrhs_transfer's num_missing): 8 bytes instead of the arrays
int64_t sampler_nfound(tpsrhs_sampler *s) {
  if (s->host_valid) return s->nfound;
  tpsrhs_operator *h = s->owner;
  unsigned long long nf = 0;
  HIP_CHECK(hipMemcpyAsync(&nf, s->d_nfound.get(), sizeof(nf), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  return static_cast<int64_t>(nf);
}

// The search grid of h's mesh for this tolerance on the device, built and uploaded at first use.
template <int DIM>
LocateGridView<DIM> device_grid(tpsrhs_operator *h, double tol) {
  if (!h->sampling) h->sampling = new tpsrhs_sampling_state();
  tpsrhs_sampling_state *ss = h->sampling;
  tpsrhs_locate_grid_dev *g = nullptr;
  for (const auto &c : ss->grids)
    if (c->tol == tol) g = c.get();
  if (!g) {
    std::unique_ptr<tpsrhs_locate_grid_dev> up(new tpsrhs_locate_grid_dev());
    up->tol = tol;
    up->host = build_locate_grid<DIM>(h->ne, h->topo.verts.data(), tol);
    up->d_lo = DevBuf<double>(up->host.lo);
    up->d_hi = DevBuf<double>(up->host.hi);
    up->d_start = DevBuf<int64_t>(up->host.start);
    up->d_list = DevBuf<int32_t>(up->host.list);
    for (auto *v : {&up->host.lo, &up->host.hi}) std::vector<double>().swap(*v);
    std::vector<int64_t>().swap(up->host.start);
    std::vector<int32_t>().swap(up->host.list);
    g = up.get();
    ss->grids.push_back(std::move(up));
  }
  return locate_grid_view<DIM>(g->host, g->d_lo.get(), g->d_hi.get(), g->d_start.get(), g->d_list.get());
}

template <int DIM>
void launch_locate(tpsrhs_operator *h, tpsrhs_sampler *s, const double *xyz, double tol) {
  constexpr int BLOCK = 64;
  const int64_t grid = (s->npts + BLOCK - 1) / BLOCK;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_sampler_create_device: more than 2^37 points");
  const LocateGridView<DIM> g = device_grid<DIM>(h, tol);
  HIP_CHECK(hipMemsetAsync(s->d_nfound.get(), 0, sizeof(unsigned long long), h->stream));
  if (grid == 0) return;
  hipLaunchKernelGGL((k_locate<DIM, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, g, h->d_verts.get(), s->npts,
                     xyz, tol, s->d_elem.get(), s->d_ref.get(), s->d_perm.get(), s->d_nfound.get());
  HIP_CHECK(hipGetLastError());
}

// a sampler of h at the DEVICE points xyz[dim][npts], located on h's stream; registered with h
tpsrhs_sampler *sampler_create_device(tpsrhs_operator *h, int64_t npts, const double *xyz, double tol, double fill) {
  if (h->ne <= 0) throw Unsupported("tpsrhs_sampler_create_device: the operator has no elements");
  const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
  std::unique_ptr<tpsrhs_sampler> s(new tpsrhs_sampler());
  s->owner = h;
  s->npts = npts;
  s->fill = fill;
  s->on_device = true;
  s->host_valid = false;
  s->d_elem = DevBuf<int32_t>(npts);
  s->d_ref = DevBuf<double>(npts * h->dim);
  s->d_perm = DevBuf<int64_t>(npts);
  s->d_nfound = DevBuf<unsigned long long>(1);
  if (h->dim == 2)
    launch_locate<2>(h, s.get(), xyz, t);
  else
    launch_locate<3>(h, s.get(), xyz, t);
  h->sampling->samplers.push_back(std::move(s));  // exists: device_grid made it
  return h->sampling->samplers.back().get();
}

void node_coordinates_device(tpsrhs_operator *h, double *xyz_out, hipStream_t stream) {
  SampleNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // as sample_field
  constexpr int BLOCK = 256;
  const int64_t grid = (h->ndofs + BLOCK - 1) / BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_node_coordinates: more than 2^39 nodes");
  if (h->dim == 2)
    hipLaunchKernelGGL((k_node_coordinates<2, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, stream, h->ndofs,
                       h->order + 1, nodes, h->d_verts.get(), xyz_out);
  else
    hipLaunchKernelGGL((k_node_coordinates<3, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, stream, h->ndofs,
                       h->order + 1, nodes, h->d_verts.get(), xyz_out);
  HIP_CHECK(hipGetLastError());
}

// is s a live sampler?  (its owner is then s->owner)
bool sampler_alive(const tpsrhs_sampler *s, const tpsrhs_operator *h) {
  tpsrhs_sampling_state *ss = h ? h->sampling : nullptr;
  return ss && sampler_find(ss, s) != ss->samplers.end();
}
}  // namespace

extern "C" {

int tpsrhs_locate_points(const tpsrhs_mesh *mesh, int64_t npts, const double *xyz, double tol, int32_t *elem_out,
                         double *ref_out) {
  const int st = locate_points(mesh, npts, xyz, tol, elem_out, ref_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_locate_points: needs a mesh of dim 2 or 3 with elem_coords, npts >= 0, non-NULL arrays and a tolerance that is a number");
  return st;
}

int tpsrhs_plane_points(const double point[3], const double normal[3], const double bb0[3], const double bb1[3], int n,
                        double *xyz_out) {
  const int st = plane_points(point, normal, bb0, bb1, n, xyz_out);
  if (st != TPSRHS_OK) return fail(st, "tpsrhs_plane_points: needs non-NULL arguments and n >= 2");
  return st;
}

int tpsrhs_sampler_create(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                          tpsrhs_sampler_handle *out) {
  if (out) *out = nullptr;
  if (!h || !out || npts < 0 || (npts > 0 && !xyz) || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_create: needs a handle, npts >= 0, the points and a tolerance that is a number");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int dim = h->dim;
    std::unique_ptr<tpsrhs_sampler> sp(new tpsrhs_sampler());
    sp->owner = h;
    sp->npts = npts;
    sp->fill = fill;
    sp->elem.assign(static_cast<size_t>(npts), -1);
    sp->ref.assign(static_cast<size_t>(npts) * dim, 0.0);
    // the operator's own host copy of the element vertices (Topology::verts, already in lexicographic corner order)
    const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
    if (dim == 2)
      locate_points_lex<2>(h->ne, h->topo.verts.data(), npts, xyz, t, sp->elem.data(), sp->ref.data());
    else
      locate_points_lex<3>(h->ne, h->topo.verts.data(), npts, xyz, t, sp->elem.data(), sp->ref.data());
    // sorted by element, ties in the caller's order, the points that were not found last
    std::vector<int64_t> perm(static_cast<size_t>(npts));
    for (int64_t i = 0; i < npts; i++) perm[static_cast<size_t>(i)] = i;
    const std::vector<int32_t> &el = sp->elem;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
      const int64_t ea = el[static_cast<size_t>(a)] < 0 ? int64_t(1) << 40 : el[static_cast<size_t>(a)];
      const int64_t eb = el[static_cast<size_t>(b)] < 0 ? int64_t(1) << 40 : el[static_cast<size_t>(b)];
      return ea < eb;
    });
    std::vector<int32_t> selem(static_cast<size_t>(npts));
    std::vector<double> sref(static_cast<size_t>(npts) * dim);
    for (int64_t k = 0; k < npts; k++) {
      const int64_t i = perm[static_cast<size_t>(k)];
      selem[static_cast<size_t>(k)] = el[static_cast<size_t>(i)];
      if (el[static_cast<size_t>(i)] >= 0) sp->nfound++;
      for (int d = 0; d < dim; d++) sref[static_cast<size_t>(k + d * npts)] = sp->ref[static_cast<size_t>(i + d * npts)];
    }
    sp->d_elem = DevBuf<int32_t>(selem);
    sp->d_ref = DevBuf<double>(sref);
    sp->d_perm = DevBuf<int64_t>(perm);
    if (!h->sampling) h->sampling = new tpsrhs_sampling_state();
    h->sampling->samplers.push_back(std::move(sp));
    *out = h->sampling->samplers.back().get();
  });
}

int tpsrhs_sampler_destroy(tpsrhs_sampler_handle s) {
  if (!s) return TPSRHS_OK;
  tpsrhs_operator *h = s->owner;
  if (!sampler_alive(s, h)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_destroy: not a sampler of a live operator");
  sampler_remove(h, s);
  return TPSRHS_OK;
}

int tpsrhs_sampler_info(tpsrhs_sampler_handle s, int64_t *npts, int64_t *nfound, int32_t *elem_out, double *ref_out) {
  if (!s) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_info: NULL sampler");
  if (!s->host_valid) {  // located on the device: the host copies come on demand
    const int st = guarded([&] { sampler_fetch(s); });
    if (st != TPSRHS_OK) return st;
  }
  if (npts) *npts = s->npts;
  if (nfound) *nfound = s->nfound;
  if (elem_out && s->npts) std::memcpy(elem_out, s->elem.data(), s->elem.size() * sizeof(int32_t));
  if (ref_out && s->npts) std::memcpy(ref_out, s->ref.data(), s->ref.size() * sizeof(double));
  return TPSRHS_OK;
}

int tpsrhs_sample(tpsrhs_sampler_handle s, int nrows, const double *field, double *out) {
  if (!s || !field || !out || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sample: needs a sampler, nrows >= 1 and non-NULL device arrays");
  tpsrhs_operator *h = s->owner;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    sample_field(h, s, nrows, field, out);
  });
}

int tpsrhs_sampler_create_device(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                                 tpsrhs_sampler_handle *out) {
  if (out) *out = nullptr;
  if (!h || !out || npts < 0 || (npts > 0 && !xyz) || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_create_device: needs a handle, npts >= 0, the device points and a tolerance that is a number");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    *out = sampler_create_device(h, npts, xyz, tol, fill);
  });
}

int tpsrhs_node_coordinates(tpsrhs_handle h, double *xyz_out) {
  if (!h || !xyz_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_node_coordinates: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    node_coordinates_device(h, xyz_out, h->stream);
  });
}

int tpsrhs_transfer(tpsrhs_handle src, tpsrhs_handle dst, int nrows, const double *field_src, double *field_dst, double tol,
                    double fill, int64_t *num_missing) {
  if (!src || !dst || !field_src || !field_dst || nrows < 1 || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer: needs two operators, nrows >= 1, non-NULL device arrays and a tolerance that is a number");
  if (src->dim != dst->dim)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer: the operators differ in dim");
  if (src->device != dst->device)
    return fail(TPSRHS_ERR_UNSUPPORTED, "tpsrhs_transfer: the operators are on different devices");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(src->device));
    const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
    tpsrhs_sampler *s = nullptr;
    {
      std::lock_guard<std::mutex> lock(g_transfer_mu);
      if (src->sampling)
        for (const tpsrhs_transfer_entry &e : src->sampling->transfers)
          if (e.dst == dst && e.tol == t) s = e.sampler;
      if (s) {
        src->sampling->num_cache_hits++;
      } else {
        // the nodes of dst, on src's stream (they depend on nothing dst's stream writes), live until they are located
        const DevBuf<double> xyz(static_cast<size_t>(dst->ndofs) * dst->dim);
        node_coordinates_device(dst, xyz.get(), src->stream);
        s = sampler_create_device(src, dst->ndofs, xyz.get(), t, fill);
        HIP_CHECK(hipStreamSynchronize(src->stream));  // once per pair: xyz is freed below
        src->sampling->transfers.push_back({dst, t, s});
        src->sampling->num_located++;
        if (std::find(g_transfer_sources.begin(), g_transfer_sources.end(), src) == g_transfer_sources.end())
          g_transfer_sources.push_back(src);
      }
    }
    s->fill = fill;
    sample_field(src, s, nrows, field_src, field_dst);
    if (dst->stream != src->stream) {  // dst's stream reads field_dst after this
      hipEvent_t ev;
      HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t e1 = hipEventRecord(ev, src->stream);
      hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(dst->stream, ev, 0) : e1;
      (void)hipEventDestroy(ev);  // released when the record has completed
      HIP_CHECK(e2);
    }
    if (num_missing) *num_missing = s->npts - sampler_nfound(s);
  });
}

int tpsrhs_transfer_stats(tpsrhs_handle src, int64_t *num_located, int64_t *num_cache_hits) {
  if (!src) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer_stats: NULL handle");
  const tpsrhs_sampling_state *ss = src->sampling;
  if (num_located) *num_located = ss ? ss->num_located : 0;
  if (num_cache_hits) *num_cache_hits = ss ? ss->num_cache_hits : 0;
  return TPSRHS_OK;
}

int tpsrhs_probe_configure(tpsrhs_handle h, tpsrhs_sampler_handle s, int64_t interval, int64_t capacity) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: NULL handle");
  if (interval < 0 || capacity < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: needs interval >= 0 (0: off) and capacity >= 0");
  const bool on = s != nullptr && interval > 0;
  if (on && capacity < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: needs capacity >= 1");
  if (on && (s->owner != h || !sampler_alive(s, h)))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: the sampler belongs to another operator");
  return guarded([&] {
    probe_off(h);
    if (!on) return;
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_probe_log log;
    log.sampler = s;
    log.cadence.interval = interval;
    log.index.capacity = capacity;
    log.d_values = DevBuf<double>(capacity * h->neq * s->npts);
    log.d_times = DevBuf<double>(capacity);
    loop_ctl(h);  // a record copies the time from there
    // complete: a call that throws above leaves the probes off.  (h->sampling exists: s is one of its samplers)
    h->sampling->probe = std::move(log);
  });
}

int tpsrhs_probe_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                      double *values_out, int reset) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_read: NULL handle");
  tpsrhs_sampling_state *ss = h->sampling;
  if (!ss || !ss->probe.sampler) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_read: probes are not configured (tpsrhs_probe_configure)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_probe_log &log = ss->probe;
    fetch_rows(h, times_out, log.d_times, log.index.nrecords, 1);
    fetch_rows(h, values_out, log.d_values, log.index.nrecords, static_cast<int64_t>(h->neq) * log.sampler->npts);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    read_index(log.index, nrecords, ndropped, iters_out, reset);
  });
}

}  // extern "C"

// ---- the wall-distance function (wall_faces.hpp, wall_distance.hpp) -----------------------------------------------------------
// After every other launch of this unit, as the integrators, the statistics and the sampling above.  No operator state: the
// face table lives on the device for the length of one call.
namespace {
template <int DIM>
void launch_wall_distance(tpsrhs_operator *h, int64_t nfaces, const double *face_xyz, double *out) {
  std::vector<double> coef;
  wd_face_table<DIM>(nfaces, face_xyz, coef);
  WdNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // the nodes of the operator's basis, as make_tables places them
  const int64_t grid = (h->ndofs + WD_BLOCK - 1) / WD_BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_wall_distance: more than 2^39 nodes");
  const char *env = std::getenv("TPSRHS_WALLDIST_CULL");
  const bool cull = !(env && env[0] == '0');
  const DevBuf<double> table(coef);
  const dim3 g(static_cast<unsigned>(grid)), b(WD_BLOCK);
  if (cull)
    hipLaunchKernelGGL((k_wall_distance<DIM, true>), g, b, 0, h->stream, h->ndofs, h->order + 1, nodes, h->d_verts.get(), nfaces,
                       table.get(), out);
  else
    hipLaunchKernelGGL((k_wall_distance<DIM, false>), g, b, 0, h->stream, h->ndofs, h->order + 1, nodes, h->d_verts.get(), nfaces,
                       table.get(), out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(h->stream));  // the table is freed on return
}
}  // namespace

extern "C" {

int tpsrhs_wall_faces(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int num_attributes, const int *attributes,
                      int64_t capacity, double *face_xyz_out, int64_t *num_faces_out) {
  const int st = wall_faces(mesh, num_bcs, bcs, num_attributes, attributes, capacity, face_xyz_out, num_faces_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_wall_faces: needs a mesh of dim 2 or 3 whose boundary records are faces of its elements, the attribute list or the boundary conditions, capacity >= 0 with its array, and num_faces_out");
  return st;
}

int tpsrhs_wall_distance(tpsrhs_handle h, int64_t num_faces, const double *face_xyz, double *distance_out) {
  if (!h || !distance_out || num_faces < 0 || (num_faces > 0 && !face_xyz))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_wall_distance: needs a handle, num_faces >= 0, the faces and the output array");
  const int64_t nval = num_faces * (int64_t(1) << (h->dim - 1)) * h->dim;
  for (int64_t i = 0; i < nval; i++)
    if (!std::isfinite(face_xyz[i]))
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_wall_distance: face coordinate " + std::to_string(i) + " is not finite");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (h->dim == 3)
      launch_wall_distance<3>(h, num_faces, face_xyz, distance_out);
    else
      launch_wall_distance<2>(h, num_faces, face_xyz, distance_out);
  });
}

}  // extern "C"

// ---- volume integrals, nodal extrema and the monitor records (quadrature_points.hpp, integrals.hpp) -------------------------
// After every other launch of this unit, as the integrators, the statistics, the sampling and the wall distance above.
namespace {
void monitor_off(tpsrhs_operator *h) {
  tpsrhs_integrals_state *is = h->integrals;
  if (!is || !is->monitor.cadence.interval) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a record may still be running
  is->monitor = tpsrhs_monitor_log();
}

void integrals_release(tpsrhs_operator *h) {
  tpsrhs_integrals_state *is = h->integrals;
  if (!is) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a reduction may still be running
  delete is;
  h->integrals = nullptr;
}

// a grid of at most INTEG_MAXBLOCKS blocks over ne elements in batches of eb: -> (blocks, elements per block)
void reduction_grid(int ne, int eb, int *blocks, int *run) {
  const int batches = (ne + eb - 1) / eb;
  const int per = std::max(1, (batches + INTEG_MAXBLOCKS - 1) / INTEG_MAXBLOCKS);
  *run = per * eb;
  *blocks = std::max(1, (batches + per - 1) / per);
}

// the state with its scratch, sized once: the grids depend on the mesh and the order only
tpsrhs_integrals_state *integrals_of(tpsrhs_operator *h) {
  if (h->integrals) return h->integrals;
  int eb = 0;
  with_dim_order(h, "tpsrhs_integrate", [&](auto dim, auto p) { eb = IntegCfg<decltype(dim)::value, decltype(p)::value>::EB; });
  std::unique_ptr<tpsrhs_integrals_state> is(new tpsrhs_integrals_state());
  is->integ_eb = eb;
  reduction_grid(h->ne, eb, &is->integ_blocks, &is->integ_run);
  const int npe = static_cast<int>(h->ndofs / std::max(h->ne, 1));
  is->stat_lpe = lanes_per_element(npe);
  reduction_grid(h->ne, 64 / is->stat_lpe, &is->stat_blocks, &is->stat_run);
  const int64_t per_row = std::max<int64_t>(2 * static_cast<int64_t>(is->integ_blocks) * eb,
                                             3 * static_cast<int64_t>(is->stat_blocks) * (64 / is->stat_lpe));
  is->d_partial = DevBuf<double>(INTEG_ROWS * per_row);
  h->integrals = is.release();
  return h->integrals;
}

template <int DIM, int P>
void launch_integrate(tpsrhs_operator *h, const tpsrhs_integrals_state *is, const QuadTab &tab, int nrows, const double *field,
                      const double *exact, int radial, double *partial) {
  typedef IntegCfg<DIM, P> C;
  hipLaunchKernelGGL((k_integrate<DIM, P>), dim3(is->integ_blocks), dim3(64), 0, h->stream, h->ne, is->integ_run, nrows, h->ndofs,
                     static_cast<int64_t>(h->ne) * C::NQD, radial, tab, h->d_verts.get(), field, exact, partial);
  HIP_CHECK(hipGetLastError());
}

// sum_out[nrows], sumsq_out[nrows] (either may be NULL) of field[nrows][NDofs] - exact[nrows][npts], on the operator's stream
void integrate_field(tpsrhs_operator *h, int nrows, const double *field, const double *exact, int radial, double *sum_out,
                     double *sumsq_out) {
  tpsrhs_integrals_state *is = integrals_of(h);
  if (h->ne == 0) {
    if (sum_out) HIP_CHECK(hipMemsetAsync(sum_out, 0, sizeof(double) * nrows, h->stream));
    if (sumsq_out) HIP_CHECK(hipMemsetAsync(sumsq_out, 0, sizeof(double) * nrows, h->stream));
    return;
  }
  QuadTab tab = {};
  const int n1 = h->order + 1, nq = quad_points_1d(h->order);
  double nodes[TPSRHS_MAXORDER + 1], wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, n1, nodes, wts);  // the nodes of the operator's basis, as make_tables places them
  gauss_legendre01(nq, tab.g, tab.w);
  for (int q = 0; q < nq; q++)
    for (int a = 0; a < n1; a++) tab.B[q * n1 + a] = lagrange(nodes, n1, a, tab.g[q]);
  const int64_t npts = static_cast<int64_t>(h->ne) * (h->dim == 3 ? nq * nq * nq : nq * nq);
  const int64_t np = static_cast<int64_t>(is->integ_blocks) * is->integ_eb;
  for (int r0 = 0; r0 < nrows; r0 += INTEG_ROWS) {  // the stream orders the launches: one scratch serves every slab of rows
    const int nr = std::min(INTEG_ROWS, nrows - r0);
    const double *f = field + r0 * h->ndofs, *ex = exact ? exact + r0 * npts : nullptr;
    with_dim_order(h, "tpsrhs_integrate", [&](auto dim, auto p) {
      launch_integrate<decltype(dim)::value, decltype(p)::value>(h, is, tab, nr, f, ex, radial, is->d_partial.get());
    });
    hipLaunchKernelGGL(k_integrate_final<1024>, dim3(1), dim3(1024), 0, h->stream, nr, np, is->d_partial.get(),
                       sum_out ? sum_out + r0 : nullptr, sumsq_out ? sumsq_out + r0 : nullptr);
    HIP_CHECK(hipGetLastError());
  }
}

void nodal_stats_field(tpsrhs_operator *h, int nrows, const double *field, double *min_out, double *max_out, double *meanabs_out) {
  tpsrhs_integrals_state *is = integrals_of(h);
  const int npe = static_cast<int>(h->ndofs / std::max(h->ne, 1));
  const int64_t np = static_cast<int64_t>(is->stat_blocks) * (64 / is->stat_lpe);
  for (int r0 = 0; r0 < nrows; r0 += INTEG_ROWS) {
    const int nr = std::min(INTEG_ROWS, nrows - r0);
    // (ne == 0: one block without elements writes the empty partials +inf, -inf, 0)
    hipLaunchKernelGGL(k_nodal_stats, dim3(is->stat_blocks, nr), dim3(64), 0, h->stream, h->ne, is->stat_run, npe, is->stat_lpe,
                       h->ndofs, field + r0 * h->ndofs, is->d_partial.get());
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_nodal_stats_final<1024>, dim3(1), dim3(1024), 0, h->stream, nr, np, h->ndofs, is->d_partial.get(),
                       min_out ? min_out + r0 : nullptr, max_out ? max_out + r0 : nullptr,
                       meanabs_out ? meanabs_out + r0 : nullptr);
    HIP_CHECK(hipGetLastError());
  }
}

// One monitor record of the device vector x, stream-ordered, or one more dropped record when the buffer is full.
void monitor_record(tpsrhs_operator *h, const double *x) {
  tpsrhs_monitor_log &log = h->integrals->monitor;
  const int64_t r = log.index.claim(log.cadence.count);
  if (r < 0) return;
  const int axisym = h->dim == 2 && h->nvel == 3;
  integrate_field(h, h->neq, x, nullptr, axisym, log.d_totals.get() + r * h->neq, nullptr);
  nodal_stats_field(h, h->neq, x, log.d_mins.get() + r * h->neq, log.d_maxs.get() + r * h->neq, nullptr);
  // {dt of the next step, time}: the loop's control block, which the variable-dt loop never has on the host
  HIP_CHECK(hipMemcpyAsync(log.d_dts.get() + r, h->loop.d_ctl.get(), sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIP_CHECK(hipMemcpyAsync(log.d_times.get() + r, h->loop.d_ctl.get() + 1, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}
}  // namespace

extern "C" {

int tpsrhs_quadrature_points(const tpsrhs_mesh *mesh, int order, double *xyz_out, double *w_out, int64_t *npts_out) {
  const int st = quadrature_points(mesh, order, xyz_out, w_out, npts_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_quadrature_points: needs a mesh of dim 2 or 3 with elem_coords, an order in 1..5 and npts_out");
  return st;
}

int tpsrhs_integrate(tpsrhs_handle h, int nrows, const double *field, const double *exact_q, int radial_weight,
                     double *sum_out, double *sumsq_out) {
  if (!h || !field || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_integrate: needs a handle, nrows >= 1 and the device field");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    integrate_field(h, nrows, field, exact_q, radial_weight ? 1 : 0, sum_out, sumsq_out);
  });
}

int tpsrhs_nodal_stats(tpsrhs_handle h, int nrows, const double *field, double *min_out, double *max_out, double *meanabs_out) {
  if (!h || !field || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_nodal_stats: needs a handle, nrows >= 1 and the device field");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    nodal_stats_field(h, nrows, field, min_out, max_out, meanabs_out);
  });
}

int tpsrhs_monitor_configure(tpsrhs_handle h, int64_t interval, int64_t capacity) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: NULL handle");
  if (interval < 0 || capacity < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: needs interval >= 0 (0: off) and capacity >= 0");
  if (interval > 0 && capacity < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: needs capacity >= 1");
  return guarded([&] {
    monitor_off(h);
    if (interval == 0) return;
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_integrals_state *is = integrals_of(h);  // with the scratch: a record allocates nothing
    tpsrhs_monitor_log log;
    log.cadence.interval = interval;
    log.index.capacity = capacity;
    log.d_times = DevBuf<double>(capacity);
    log.d_dts = DevBuf<double>(capacity);
    log.d_totals = DevBuf<double>(capacity * h->neq);
    log.d_mins = DevBuf<double>(capacity * h->neq);
    log.d_maxs = DevBuf<double>(capacity * h->neq);
    loop_ctl(h);  // a record copies dt and the time from there
    is->monitor = std::move(log);  // complete: a call that throws above leaves the monitor off
  });
}

int tpsrhs_monitor_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                        double *dts_out, double *totals_out, double *mins_out, double *maxs_out, int reset) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_read: NULL handle");
  tpsrhs_integrals_state *is = h->integrals;
  if (!is || !is->monitor.cadence.interval)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_read: the monitor is not configured (tpsrhs_monitor_configure)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_monitor_log &log = is->monitor;
    const int64_t n = log.index.nrecords;
    fetch_rows(h, times_out, log.d_times, n, 1);
    fetch_rows(h, dts_out, log.d_dts, n, 1);
    fetch_rows(h, totals_out, log.d_totals, n, h->neq);
    fetch_rows(h, mins_out, log.d_mins, n, h->neq);
    fetch_rows(h, maxs_out, log.d_maxs, n, h->neq);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    read_index(log.index, nrecords, ndropped, iters_out, reset);
  });
}

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
    if (!h->vis_fields) {  // the passes of this family: a shared object of its own, loaded at the first call
      const tpsrhs_perfect_mixture &mx = h->phys.mixture;
      const int tr = (h->phys.transport_model == TPSRHS_CONSTANT)
                         ? TRANSPORT_CONSTANT
                         : (h->phys.transport_model == TPSRHS_ARGON_MINIMAL ? TRANSPORT_ARGON_MINIMAL : TRANSPORT_ARGON_MIXTURE);
      const char *geo = (h->dim == 3) ? "3d" : (h->nvel > h->dim ? "axi" : "2d");
      const std::string unit = std::string("plasma_vis_") + geo + "_n" + std::to_string(mx.num_species) + (mx.ambipolar ? "a" : "");
      char msg[512] = {0};
      const int rc = load_family(unit)(h, mx.two_temperature ? 1 : 0, tr, msg, static_cast<int>(sizeof msg));
      if (rc != TPSRHS_OK || !h->vis_fields) throw Unsupported(std::string("visualization fields: ") + msg);
    }
    HIP_CHECK(hipSetDevice(h->device));
    h->launch(h, x, nullptr, true);  // rhsOperator->updateGradients(*U, false): Up and gradUp of x
    const VisRows rows = {l.Xsp, l.Ysp, l.nsp_, l.FluxTrns, l.diffVel, l.SrcTrns, l.SpeciesTrns, l.rxn};
    h->vis_fields(h, rows, x, out);
  });
}

}  // extern "C"
