/*
 * tpsrhs.h -- C ABI of the MI355X-native replacement for the explicit DG right-hand side of the
 * TPS compressible solver (M2ulPhyS): RHSoperator::Mult.
 *
 * Every entry point names the reference interface it replaces (paths relative to the pecos/tps
 * source tree).  Only plain C types cross this boundary: pointers, sizes, PODs.  No torch, no
 * MFEM, no C++ types.
 *
 * Conventions shared with the reference (part of the contract):
 *   - state vectors are "byNODES": U[n + eq * NDofs]            (src/M2ulPhyS.cpp:575-579)
 *   - gradients:  gradUp[n + eq*NDofs + d*num_equation*NDofs]   (src/rhs_operator.cpp:521)
 *   - DG L2 space: dof n = element * dofs_per_element + local,  local = i + j*(p+1) + k*(p+1)^2
 *     (lexicographic in the element's reference frame; MFEM L2_{Quadrilateral,Hexahedron}Element)
 *   - conserved state  [rho, rho u (nvel), rho E, rho Y_sp (active) ..., (rho e_e)]
 *     primitive state  [rho, u (nvel), T_h, n_sp (active) ..., (T_e)]   (src/equation_of_state.cpp:679-700)
 *   - element vertex order is MFEM's (quad: counter-clockwise; hex: bottom ccw then top ccw).
 */
#ifndef TPSRHS_H_
#define TPSRHS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- capacity limits: src/dataStructures.hpp:41-65 (gpudata::MAX*) ------------------------- */
#define TPSRHS_MAXDIM 3
#define TPSRHS_MAXSPECIES 8
#define TPSRHS_MAXEQUATIONS (TPSRHS_MAXDIM + 2 + TPSRHS_MAXSPECIES)
#define TPSRHS_MAXREACTIONS 34
#define TPSRHS_MAXCHEMPARAMS 3
#define TPSRHS_MAXTABLE 1000
#define TPSRHS_MAXORDER 5 /* MAXDOFS = 216 = hex p=5 */

/* ---- status codes (the reference uses assert/exit/MPI_Abort; src/equation_of_state.cpp:643-650) */
enum tpsrhs_status {
  TPSRHS_OK = 0,
  TPSRHS_ERR_INVALID_ARGUMENT = 1,
  TPSRHS_ERR_UNSUPPORTED = 2, /* a configuration outside the built hot-path scope */
  TPSRHS_ERR_MESH = 3,        /* inconsistent connectivity / boundary faces */
  TPSRHS_ERR_DEVICE = 4,      /* HIP runtime error */
  TPSRHS_ERR_NO_DEVICE = 5,   /* no gfx950 device visible: the library never falls back to CPU */
  TPSRHS_ERR_HALO = 6         /* halo-exchange callback failed */
};

/* ---- enums with the reference's names and values: src/dataStructures.hpp:67-196 -------------- */
enum tpsrhs_equations { TPSRHS_EULER = 0, TPSRHS_NS = 1, TPSRHS_NS_PASSIVE = 2 };
enum tpsrhs_working_fluid { TPSRHS_DRY_AIR = 0, TPSRHS_USER_DEFINED = 1, TPSRHS_LTE_FLUID = 2 };
enum tpsrhs_transport_model {
  TPSRHS_ARGON_MINIMAL = 0,
  TPSRHS_ARGON_MIXTURE = 1,
  TPSRHS_CONSTANT = 2,
  TPSRHS_LTE_TRANSPORT = 3,
  TPSRHS_MIXING_LENGTH = 4
};
enum tpsrhs_reaction_model {
  TPSRHS_ARRHENIUS = 0,
  TPSRHS_HOFFERTLIEN = 1,
  TPSRHS_TABULATED_RXN = 2,
  TPSRHS_GRIDFUNCTION_RXN = 3,
  TPSRHS_RADIATIVE_DECAY = 4
};
enum tpsrhs_radiation_model { TPSRHS_NONE_RAD = 0, TPSRHS_NET_EMISSION = 1 };
enum tpsrhs_gas_params {
  TPSRHS_SPECIES_MW = 0,
  TPSRHS_SPECIES_CHARGES = 1,
  TPSRHS_FORMATION_ENERGY = 2,
  TPSRHS_SPECIES_DEGENERACY = 3,
  TPSRHS_NUM_GASPARAMS = 4
};
enum tpsrhs_gas_coll {
  TPSRHS_CLMB_ATT = 0,
  TPSRHS_CLMB_REP = 1,
  TPSRHS_AR_AR1P = 2,
  TPSRHS_AR_E = 3,
  TPSRHS_AR_AR = 4,
  TPSRHS_NONE_ARGCOLL = 5
};
enum tpsrhs_bc_category { TPSRHS_INLET = 0, TPSRHS_OUTLET = 1, TPSRHS_WALL = 2 };
enum tpsrhs_inlet_type {
  TPSRHS_UNI_DENS_VEL = 0,
  TPSRHS_INTERPOLATE = 1,
  TPSRHS_SUB_DENS_VEL = 2,
  /* density and velocity RELATIVE TO THE INLET FACE (src/inletBC.cpp:453-464, 758-864; "subsonicFaceBasedX/Y/Z"): data =
   * {rho, U_normal (into the domain), U_tangent, unused, active species ...}; the face frame is the inward unit normal
   * made orthogonal to the global x / y / z axis, the axis itself, and their cross product.  3-D only (the reference's
   * frame has three components). */
  TPSRHS_SUB_DENS_VEL_FACE_X = 3,
  TPSRHS_SUB_DENS_VEL_FACE_Y = 4,
  TPSRHS_SUB_DENS_VEL_FACE_Z = 5,
  TPSRHS_SUB_DENS_VEL_NR = 6,   /* non-reflecting, density and velocity (src/inletBC.cpp:576-727) */
  TPSRHS_SUB_VEL_CONST_ENT = 7  /* non-reflecting, velocity, constant entropy (same routine, L2 = 0) */
};
enum tpsrhs_outlet_type {
  TPSRHS_SUB_P = 0,
  TPSRHS_SUB_P_NR = 2,     /* non-reflecting pressure outlet (src/outletBC.cpp:573-728) */
  TPSRHS_SUB_MF_NR = 3,    /* non-reflecting mass-flow outlet (src/outletBC.cpp:739-892) */
  TPSRHS_SUB_MF_NR_PW = 4  /* point-wise variant (src/outletBC.cpp:894-1027) */
};
enum tpsrhs_wall_type {
  TPSRHS_INV = 0,
  TPSRHS_SLIP = 1,
  TPSRHS_VISC_ADIAB = 2,
  TPSRHS_VISC_ISOTH = 3,
  TPSRHS_VISC_GNRL = 4
};
enum tpsrhs_thermal_condition { TPSRHS_ADIAB = 0, TPSRHS_ISOTH = 1, TPSRHS_SHTH = 2, TPSRHS_NONE_THMCND = 3 };
enum tpsrhs_basis_type { TPSRHS_BASIS_GAUSS_LEGENDRE = 0, TPSRHS_BASIS_GAUSS_LOBATTO = 1 };

/* ---- mesh: what the reference takes from mfem::ParMesh (src/M2ulPhyS.cpp:296-470) ------------ */
typedef struct tpsrhs_mesh {
  int dim;          /* 2 (quadrilaterals) or 3 (hexahedra) */
  int num_vertices; /* topological vertices (periodic images identified) */
  int num_elements;
  const int *elem_vertices;   /* [num_elements * 2^dim] topological vertex ids, MFEM order */
  const double *elem_coords;  /* [num_elements * 2^dim * dim] coordinates of each element's own
                                 vertices (order-1 discontinuous nodes: periodic meshes keep their
                                 geometry, as with mfem::Mesh::MakePeriodic) */
  int num_bdr_faces;
  const int *bdr_vertices;    /* [num_bdr_faces * 2^(dim-1)] */
  const int *bdr_attributes;  /* [num_bdr_faces], matched to tpsrhs_bc::attribute */
  /* faces shared with other ranks (mfem::ParMesh shared faces; src/rhs_operator.cpp:716-773).
   * Listed in the same order on both ranks of a pair, grouped by neighbour rank. */
  int num_shared_faces;
  const int *shared_vertices;       /* [num_shared_faces * 2^(dim-1)] local vertex ids, ordered by
                                       ascending GLOBAL vertex id (identical physical order on both
                                       sides) */
  const int *shared_neighbor_rank;  /* [num_shared_faces] */
  /* Optional: [num_elements] mfem::Mesh::GetElementSize(e, 1) (the smallest singular value of the Jacobian at the
   * element centre), the grid scale of the sub-grid scale models (src/rhs_operator.cpp:154,
   * src/face_integrator.cpp:253).  NULL: the library computes it from elem_coords. */
  const double *elem_size;
} tpsrhs_mesh;

/* ---- discretisation: [flow] order/basisType/integrationRule (src/M2ulPhyS.cpp:557-579,2670) -- */
typedef struct tpsrhs_disc {
  int order;             /* polynomial order p, 1..TPSRHS_MAXORDER */
  int basis_type;        /* tpsrhs_basis_type (reference basisType) */
  int int_rule_type;     /* 0 Gauss-Legendre, 1 Gauss-Lobatto (reference integrationRule) */
  int axisymmetric;      /* dim must be 2; nvel = 3 */
  int use_bc_in_grad;    /* boundaryConditions/useBCinGrad (src/M2ulPhyS.cpp:3480) */
  int use_roe;           /* flow/useRoe (src/M2ulPhyS.cpp:2676): RiemannSolverTPS::Eval_Roe on interior faces and
                          * inviscid walls (src/riemann_solver.cpp:66-72,117-206); the reference's formula is
                          * 2-D, single-species, not axisymmetric -- anything else: TPSRHS_ERR_UNSUPPORTED */
  double ref_length;     /* flow/refLength (src/M2ulPhyS.cpp:2677), relaxation length of the non-reflecting
                          * boundary conditions; 0 = the reference's default 1.0 */
} tpsrhs_disc;

/* ---- physics parameter blocks: the PODs of src/dataStructures.hpp:537-729 -------------------- */
typedef struct tpsrhs_dry_air { /* DryAirInput + SutherlandData + visc multipliers */
  double specific_heat_ratio;   /* 1.4     (src/M2ulPhyS.cpp:2882) */
  double gas_constant;          /* 287.058 (src/M2ulPhyS.cpp:2883) */
  double visc_mult;             /* flow/viscosityMultiplier */
  double bulk_visc_mult;        /* flow/bulkViscosityMultiplier */
  double sutherland_C1;         /* 1.458e-6 */
  double sutherland_S0;         /* 110.4 */
  double sutherland_Pr;         /* 0.71 */
} tpsrhs_dry_air;

typedef struct tpsrhs_perfect_mixture { /* PerfectMixtureInput */
  int num_species;
  int is_electron_included;
  int ambipolar;
  int two_temperature;
  double gas_params[TPSRHS_MAXSPECIES * TPSRHS_NUM_GASPARAMS]; /* [sp + param * num_species] */
  double molar_cv[TPSRHS_MAXSPECIES];                          /* J/(mol K) */
} tpsrhs_perfect_mixture;

typedef struct tpsrhs_constant_transport { /* constantTransportData */
  double viscosity;
  double bulk_viscosity;
  double diffusivity[TPSRHS_MAXSPECIES];
  double thermal_conductivity;
  double electron_thermal_conductivity;
  double mt_freq[TPSRHS_MAXSPECIES];
  int electron_index;
} tpsrhs_constant_transport;

typedef struct tpsrhs_gas_transport { /* GasTransportInput */
  int neutral_index;
  int ion_index;
  int electron_index;
  int third_order_k_electron;
  int collision_index[TPSRHS_MAXSPECIES * TPSRHS_MAXSPECIES]; /* tpsrhs_gas_coll, [i + j*nsp] */
  int multiply;
  double flux_trns_multiplier[4];
  double spcs_trns_multiplier[1];
  double diff_mult;
  double mobil_mult;
} tpsrhs_gas_transport;

typedef struct tpsrhs_table { /* TableInput (order 1 interpolation only, src/table.cpp:52-110) */
  int n_data;
  const double *x_data;
  const double *f_data;
  int x_log_scale;
  int f_log_scale;
} tpsrhs_table;

typedef struct tpsrhs_chemistry { /* ChemistryInput */
  int num_reactions;
  int electron_index;
  double reaction_energies[TPSRHS_MAXREACTIONS];
  int detailed_balance[TPSRHS_MAXREACTIONS];
  int16_t reactant_stoich[TPSRHS_MAXSPECIES * TPSRHS_MAXREACTIONS]; /* [sp + r * num_species] */
  int16_t product_stoich[TPSRHS_MAXSPECIES * TPSRHS_MAXREACTIONS];
  int reaction_models[TPSRHS_MAXREACTIONS];                          /* tpsrhs_reaction_model */
  double equilibrium_constant_params[TPSRHS_MAXCHEMPARAMS * TPSRHS_MAXREACTIONS];
  double rate_params[TPSRHS_MAXCHEMPARAMS * TPSRHS_MAXREACTIONS];    /* A, b, E of the model */
  tpsrhs_table rate_tables[TPSRHS_MAXREACTIONS];                     /* TABULATED_RXN only */
  double minimum_temperature;
} tpsrhs_chemistry;

typedef struct tpsrhs_radiation { /* RadiationInput */
  int model; /* tpsrhs_radiation_model */
  tpsrhs_table nec_table;
} tpsrhs_radiation;

/* Fluxes: sub-grid scale model ([flow] sgsModel / sgsModelConstant / sgsFloor, src/M2ulPhyS.cpp:2689-2699,
 * src/fluxes.cpp:513-665) and the planar viscous sponge ([viscosityMultiplierFunction], src/M2ulPhyS.cpp:2788-2808,
 * src/fluxes.cpp:669-688).  The sub-grid scale models: dry air, 3-D (the reference's strain tensor indexes three
 * directions).  The viscous sponge: dry air planar 2-D and 3-D, and every 2-D formulation with the heavy kernel
 * interface -- axisymmetric dry air and table gas, the mixtures planar and axisymmetric (there it also scales the
 * diffusion velocities of the active species, src/fluxes.cpp:240-245).  Gauss-Legendre pair; anything else:
 * TPSRHS_ERR_UNSUPPORTED. */
enum tpsrhs_sgs_model { TPSRHS_SGS_NONE = 0, TPSRHS_SGS_SMAGORINSKY = 1, TPSRHS_SGS_SIGMA = 2 };
typedef struct tpsrhs_sgs {
  int model_type;      /* tpsrhs_sgs_model */
  double model_const;  /* 0: the reference's default, 0.12 (Smagorinsky) / 0.135 (sigma) */
  double model_floor;  /* sgsFloor */
} tpsrhs_sgs;
typedef struct tpsrhs_visc_sponge { /* viscositySpongeData (src/M2ulPhyS.cpp:583-600) */
  int enabled;
  double normal[3], point[3]; /* the normal is normalised, as the constructor of every CPU build of the reference does
                               * (src/fluxes.cpp:77-90; its device constructor :98-125 does not) */
  double width, ratio;
} tpsrhs_visc_sponge;

/* WorkingFluid::LTE_FLUID: the local-thermodynamic-equilibrium table gas, LteMixture + LteTransport
 * (src/lte_mixture.cpp, src/lte_transport_properties.cpp) with ONE-DIMENSIONAL tables in the temperature
 * (`flow/lte/table_dim = 1`, the variant of the reference's device build, src/M2ulPhyS.cpp:164-255: the columns of its
 * "T_energy_R_c" and "T_mu_kappa_sigma" datasets; linear scales).  One species, num_equation = nvel + 2; the inverse
 * table T(e) is the energy table with abscissae and values swapped, as the reference builds it (:193-200), so the
 * energies must increase with the temperature.  The two-dimensional (T, rho) tables of the reference's CPU build
 * (`flow/lte/table_dim = 2`, its default) are tpsrhs_lte2d below.  The radiation sink of SourceTerm
 * (src/source_term.cpp:207-209) is tpsrhs_physics::radiation; the electric conductivity table feeds the
 * plasma-conductivity side output of SourceTerm (:196): tpsrhs_get_plasma_conductivity.  Every table must have linear
 * scales (x_log_scale = f_log_scale = 0, as the reference hard-codes): TPSRHS_ERR_INVALID_ARGUMENT otherwise.
 * Built for the axisymmetric formulation (the reference's LTE inputs, test/inputs/plasma.lte1d.ini), Gauss-Legendre
 * pair; anything else: TPSRHS_ERR_UNSUPPORTED. */
typedef struct tpsrhs_lte { /* LteMixtureInput + the TableInputs of src/M2ulPhyS.cpp:176-255 */
  tpsrhs_table energy_table;                /* T -> specific internal energy e [J/kg] */
  tpsrhs_table gas_constant_table;          /* T -> mixture gas constant R [J/(kg K)], p = rho R T */
  tpsrhs_table sound_speed_table;           /* T -> c [m/s] */
  tpsrhs_table viscosity_table;             /* T -> mu [Pa s] */
  tpsrhs_table conductivity_table;          /* T -> kappa [W/(m K)] */
  tpsrhs_table electric_conductivity_table; /* T -> sigma [S/m] */
} tpsrhs_lte;

/* A two-dimensional table on a tensor grid, bilinear: GslTableInterpolator2D with gsl_interp2d_bilinear
 * (src/table.cpp:170-260).  Host pointers, copied at create.  f[j * nx + i] belongs to (x[i], y[j]), the storage of the
 * reference (:195-207).  Both axes strictly increasing, nx >= 2, ny >= 2, finite data: TPSRHS_ERR_INVALID_ARGUMENT otherwise.
 * Cell i holds x[i] <= x < x[i+1]; the last abscissa belongs to the last cell.  With t = (x - x_i) / dx, u = (y - y_j) / dy:
 *   z   = (1-t)(1-u) z00 + t(1-u) z10 + (1-t)u z01 + t u z11
 *   z_x = (-(1-u) z00 + (1-u) z10 - u z01 + u z11) / dx,   z_y likewise with t and u swapped.
 * ONE DEPARTURE from the reference: outside the table GSL raises a domain error, which aborts the program.  This library
 * clamps the cell index to the end cell, i.e. extrapolates linearly from it, as the reference's own one-dimensional tables do
 * (src/table.cpp:69-72). */
typedef struct tpsrhs_table2d {
  int nx, ny;
  const double *x, *y, *f;
} tpsrhs_table2d;

/* WorkingFluid::LTE_FLUID with TWO-DIMENSIONAL tables (`flow/lte/table_dim = 2`, the reference's default,
 * src/M2ulPhyS.cpp:166, test/inputs/plasma.lte2d.ini), which the reference itself refuses on a GPU (:168-170).
 * enabled = 0: tpsrhs_physics::lte is the gas (one-dimensional tables).  enabled = 1: these tables are, and `lte` is ignored.
 * Same kernels, entry points and scope as the one-dimensional gas: axisymmetric formulation, Gauss-Legendre pair; anything
 * else TPSRHS_ERR_UNSUPPORTED.  Every look-up takes the density of the state it is given.  The net-emission table of
 * tpsrhs_physics::radiation stays one-dimensional in T.  `energy`, `gas_constant` and `sound_speed` must share their axes
 * (nx, ny, x, y equal: the columns of one thermo file, as the reference reads them), `viscosity` and `conductivity` likewise
 * (one transport file) -- one cell search serves the tables of a file; tables that do not: TPSRHS_ERR_UNSUPPORTED.
 * `temperature` and `electric_conductivity` may have axes of their own.  `energy` must increase with T on every density line (the Newton
 * iteration divides by de/dT): TPSRHS_ERR_INVALID_ARGUMENT otherwise. */
typedef struct tpsrhs_lte2d {
  int enabled;
  tpsrhs_table2d energy;                /* (T, rho) -> e [J/kg]         thermo file column 3 (src/lte_mixture.cpp:48-58) */
  tpsrhs_table2d gas_constant;          /* (T, rho) -> R [J/(kg K)]     column 6 */
  tpsrhs_table2d sound_speed;           /* (T, rho) -> c [m/s]          column 8 */
  tpsrhs_table2d temperature;           /* (e, rho) -> T: the e_rev_table (:60-64); only the first guess of the Newton iteration */
  tpsrhs_table2d viscosity;             /* (T, rho) -> mu [Pa s]        (src/lte_transport_properties.cpp:38-51) */
  tpsrhs_table2d conductivity;          /* (T, rho) -> kappa [W/(m K)] */
  tpsrhs_table2d electric_conductivity; /* (T, rho) -> sigma [S/m] */
} tpsrhs_lte2d;

typedef struct tpsrhs_physics {
  int eq_system;        /* tpsrhs_equations */
  int working_fluid;    /* tpsrhs_working_fluid */
  tpsrhs_dry_air dry_air;
  tpsrhs_perfect_mixture mixture;
  int transport_model;  /* tpsrhs_transport_model (USER_DEFINED fluids) */
  tpsrhs_constant_transport constant_transport;
  tpsrhs_gas_transport gas_transport;
  tpsrhs_chemistry chemistry;
  tpsrhs_radiation radiation;
  tpsrhs_sgs sgs;
  tpsrhs_visc_sponge visc_sponge;
  tpsrhs_lte lte;       /* LTE_FLUID only */
  tpsrhs_lte2d lte2d;   /* LTE_FLUID only; the last member: no offset of an earlier one depends on it */
} tpsrhs_physics;

/* ---- boundary conditions: [boundaryConditions/...] (src/M2ulPhyS.cpp:3480-3700) --------------- */
typedef struct tpsrhs_bc {
  int attribute; /* mesh boundary attribute ("patch") */
  int category;  /* tpsrhs_bc_category */
  int type;      /* tpsrhs_inlet_type | tpsrhs_outlet_type | tpsrhs_wall_type */
  /* inlet SUB_DENS_VEL: rho, u, v, w, then active species (src/inletBC.cpp:729-757)
   * outlet SUB_P:       p                                  (src/outletBC.cpp:731-737)
   * non-reflecting types (perfect gas only, as the reference's characteristic algebra):
   *   inlet SUB_DENS_VEL_NR / SUB_VEL_CONST_ENT: rho, u, v, w;  outlet SUB_P_NR: p;  SUB_MF_NR(_PW): mass flow;
   *   for all of them data[4..6] = the patch tangent `tangent1` the reference takes from its first boundary
   *   face (src/outletBC.cpp:160-172; all zero: the library takes an edge of its own first face of the patch --
   *   the boundary term does not depend on the choice for a planar patch) and data[7] = the total patch area
   *   `area_` over all ranks (src/outletBC.cpp:329-343; mass-flow types only).
   * wall INV, SLIP, VISC_ADIAB: no data                    (src/wallBC.cpp:277-469)
   * wall VISC_ISOTH:    T_wall                             (src/wallBC.cpp:96-111)
   * wall VISC_GNRL:     T_h, T_e, heavy thermal condition, electron thermal condition (WallData,
   *                     src/dataStructures.hpp:564-570; tpsrhs_thermal_condition)  (src/wallBC.cpp:112-148) */
  double data[4 + TPSRHS_MAXSPECIES];
} tpsrhs_bc;

/* ---- runtime: device, stream and the halo-exchange hook -------------------------------------- */
/* Called twice per Mult on a partitioned mesh, where the reference posts MPI_Isend/Irecv of
 * neighbour-element data (src/rhs_operator.cpp:775-831).  `send` and `recv` are DEVICE buffers of
 * doubles; segment r of each (offsets[r] .. offsets[r+1]) goes to / comes from neighbor_ranks[r].
 * The callback must enqueue or complete the exchange so that `recv` is valid for work submitted to
 * `stream` after it returns (RCCL send/recv on that stream, or a blocking GPU-aware MPI call).
 * phase 0: U/Up face traces, phase 1: viscous normal-flux traces.  Return 0 on success. */
typedef int (*tpsrhs_halo_fn)(void *ctx, int phase, const double *send, double *recv,
                              int num_neighbors, const int *neighbor_ranks,
                              const int64_t *send_offsets, const int64_t *recv_offsets, void *stream);

/* Reduction over the ranks of the job (`op`: tpsrhs_reduce_op), in place, of `count` doubles in DEVICE memory,
 * ordered on `stream`.  SUM: the MPI_Allreduce of the boundary means of the non-reflecting inlet/outlet conditions
 * (src/outletBC.cpp:533-540, src/inletBC.cpp:548-555; one call per Mult for all such patches together --
 * ranks without faces on a patch contribute zeros, so the job-wide sum equals the reference's
 * per-patch communicator), and of the plane sums of a mixed-out sponge zone (src/forcing_terms.cpp:732-735).
 * MIN: the MPI_Allreduce of the time step in tpsrhs_advance (src/M2ulPhyS.cpp:2013-2016).  Return 0 on success.
 * `stream` may be NULL: that is the legacy default stream, and the implementation must order its work THERE (a
 * torch-based hook maps it to torch.cuda.default_stream -- torch.cuda.ExternalStream(0) is a different stream). */
enum tpsrhs_reduce_op { TPSRHS_REDUCE_SUM = 0, TPSRHS_REDUCE_MIN = 1 };
typedef int (*tpsrhs_reduce_fn)(void *ctx, double *values, int count, int op, void *stream);

typedef struct tpsrhs_runtime {
  int device;            /* HIP device ordinal (reference: rank % numGpusPerRank, src/tps.cpp:196) */
  void *stream;          /* hipStream_t for all work of this operator, NULL = default stream */
  tpsrhs_halo_fn halo;   /* required when mesh.num_shared_faces > 0 */
  void *halo_ctx;
  tpsrhs_reduce_fn reduce; /* required when mesh.num_shared_faces > 0 and a non-reflecting patch exists, a mixed-out
                            * sponge zone is set, or tpsrhs_advance runs with a variable time step */
  void *reduce_ctx;
} tpsrhs_runtime;

typedef struct tpsrhs_operator *tpsrhs_handle;

/* Replaces the RHSoperator constructor and everything it precomputes (Me_inv, Ke, face tables:
 * src/rhs_operator.cpp:39-322, src/gradients.cpp:84-133, src/M2ulPhyS.cpp:816-1486). */
int tpsrhs_create(const tpsrhs_mesh *mesh, const tpsrhs_disc *disc, const tpsrhs_physics *physics,
                  int num_bcs, const tpsrhs_bc *bcs, const tpsrhs_runtime *runtime,
                  tpsrhs_handle *out);

/* RHSoperator::~RHSoperator (src/rhs_operator.cpp:324-341). */
int tpsrhs_destroy(tpsrhs_handle h);

/* RHSoperator::Mult(const Vector &x, Vector &y) const  (src/rhs_operator.hpp:157,
 * src/rhs_operator.cpp:343-464).  x, y: DEVICE pointers, num_equation*NDofs doubles, byNODES.
 * `time` is TimeDependentOperator::GetTime() (src/rhs_operator.cpp:459).  When max_char_speed is
 * non-NULL the rank-local maximum of |u|+c over the nodes (src/rhs_operator.cpp:549-553) is copied
 * to that HOST address (this synchronises the stream; pass NULL to stay asynchronous; the
 * MPI_Allreduce(MAX) of src/rhs_operator.cpp:558 is the caller's). */
int tpsrhs_mult(tpsrhs_handle h, const double *x, double *y, double time, double *max_char_speed);

/* Same with HOST vectors (copies over PCIe; for the MFEM adapter when Vectors live on the host). */
int tpsrhs_mult_host(tpsrhs_handle h, const double *x, double *y, double time,
                     double *max_char_speed);

/* RHSoperator::updatePrimitives + updateGradients (src/rhs_operator.cpp:623-713): refresh the
 * operator-owned Up / gradUp from x (device pointer). */
int tpsrhs_update_gradients(tpsrhs_handle h, const double *x);

/* Up / gradUp grid functions Mult refreshes as a side effect (src/rhs_operator.hpp:74-77):
 * copy the operator-owned device arrays to a DEVICE buffer (neq*NDofs / dim*neq*NDofs doubles). */
int tpsrhs_get_primitives(tpsrhs_handle h, double *up_out);
int tpsrhs_get_gradients(tpsrhs_handle h, double *gradup_out);
/* SourceTerm's side output (src/source_term.cpp:125-199): the `plasma_conductivity_` grid function that the EM solver of
 * the cycle-avg-joule-coupled runs reads between flow steps (the other half of that coupling is
 * tpsrhs_set_joule_heating).  sigma at every node of the state `x` (DEVICE, the layout of tpsrhs_mult; species rows clamped
 * at zero as SourceTerm does): the SrcTrns::ELECTRIC_CONDUCTIVITY of the transport model's source properties --
 * mixtures: computeMixtureElectricConductivity(mobility, n) * MOLARELECTRONCHARGE (src/transport_properties.cpp:421-428,
 * src/gas_transport.cpp:725-739, 1455-1463); table gas: max(sigma(T), 1) (src/lte_transport_properties.cpp:109-126).
 * `sigma_out`: NDofs doubles, DEVICE memory, ordered on the operator's stream.  TPSRHS_ERR_UNSUPPORTED where the
 * reference does not store it: dry air (no SourceTerm) and reacting mixtures that are not ambipolar (:178-197). */
int tpsrhs_get_plasma_conductivity(tpsrhs_handle h, const double *x, double *sigma_out);

/* A->Height() (src/rhs_operator.cpp:49), vfes->GetNDofs(), num_equation. */
/* Point-wise closures of the gas model on the device, for n conserved states U[eq * n + i] (device pointers,
 * synchronous): the public GasMixture methods the reference's unit tests call directly --
 * GetPrimitivesFromConservatives (src/equation_of_state.cpp:321-335,679-700), ComputePressure (:605-628 of the
 * header, :1044-1062), ComputeSpeedOfSound (:337-348,1405-1432; test/test_speed_of_sound.cpp:84-93),
 * ComputeMaxCharSpeed (:278-292,1359-1373).  out: [neq][n] for the primitives, [n] otherwise. */
enum tpsrhs_point_quantity {
  TPSRHS_POINT_PRIMITIVES = 0,
  TPSRHS_POINT_PRESSURE = 1,
  TPSRHS_POINT_SOUND_SPEED = 2,
  TPSRHS_POINT_MAX_CHAR_SPEED = 3
};
int tpsrhs_eval_pointwise(tpsrhs_handle h, int quantity, int64_t n, const double *U, double *out);

/* TableInterpolator::eval of a LinearTable (src/table.cpp:52-110; test/test_table.cpp:104-121) on the device
 * for n abscissae (x, f: device pointers; the table itself is host data as in tpsrhs_chemistry).  Synchronous. */
int tpsrhs_table_eval(const tpsrhs_table *table, int64_t n, const double *x, double *f);
/* A two-dimensional table (tpsrhs_table2d) at n points (x[i], y[i]): what = 0 the value, 1 d/dx, 2 d/dy.  Host pointers;
 * runs on the host, needs no device; the text the kernels of the two-dimensional table gas look their tables up with. */
int tpsrhs_table2d_eval(const tpsrhs_table2d *table, int what, int64_t n, const double *x, const double *y, double *out);

/* Diagnostic: the elementary functions the device closures are built on (tps_amd/csrc/fastmath.hpp; they replace
 * the libm calls of the reference's point physics -- pow / exp / log of src/collision_integrals.cpp:53-201,
 * src/reaction.cpp:41-83 -- and its divisions / sqrt), evaluated on the device for n arguments (device pointers,
 * synchronous), so that their accuracy is a tested number: 0 exp, 1 exp without the range check, 2 log,
 * 3 log of a positive finite argument, 4 reciprocal, 5 sqrt, 6 reciprocal sqrt. */
int tpsrhs_math_eval(int function, int64_t n, const double *x, double *y);

/* Diagnostic: the eight Coulomb collision fits of the third-order electron conductivity (att11, rep22, rep23, rep24,
 * att12 .. att15 of src/collision_integrals.cpp:53-115) without their factor 1 / Tp^2, c0 log(1 + c1 e^(c2 x))^c3, at
 * n arguments x = ln Tp; out[f * n + i] (x, out: device pointers, synchronous).  Route 0: the formulas through the
 * device's exp / log; 1: the polynomial table of the 3-D p = 3 sweeps (tps_amd/csrc/coulomb_table.hpp) with wave-uniform
 * coefficient loads; 2: the same table read lane by lane; 3: the table through a window of two consecutive intervals in
 * LDS that a 64-lane wave owns (the sweeps' route, which holds three or four): four one-wave blocks stride over the chunks of 64 arguments, chunk c
 * goes to block c % 4, and a wave carries its window from one chunk to its next -- reloaded only when the lowest interval
 * of the chunk is outside it; lanes above the window read lane by lane.  Arguments off the table (and NaN) take route 0 in
 * every route.  Routes 1, 2 and 3 agree bit for bit. */
int tpsrhs_coulomb_eval(int route, int64_t n, const double *x, double *out);

int64_t tpsrhs_height(tpsrhs_handle h);
int64_t tpsrhs_num_dofs(tpsrhs_handle h);
int tpsrhs_num_equation(tpsrhs_handle h);

/* Per-kernel device time, averaged over the tpsrhs_mult calls since timing was enabled (at most the
 * last 128), measured with hipEvents on the operator's stream (enabling adds event records only;
 * reading synchronises the stream).  names[i] are static strings.  Returns the number of kernels
 * written (<= capacity).  With a halo callback the k_gradient / k_flux intervals include it. */
int tpsrhs_enable_kernel_timing(tpsrhs_handle h, int enable);
int tpsrhs_kernel_times(tpsrhs_handle h, int capacity, const char **names, double *milliseconds);
/* Device time of each recorded tpsrhs_mult call, first kernel start to last kernel end (the same event sets):
 * what the median of SURVEY 8(d) is taken over.  Returns the number of calls written (<= capacity, <= 128). */
int tpsrhs_mult_times(tpsrhs_handle h, int capacity, double *milliseconds);

/* Algorithmic HBM bytes one tpsrhs_mult moves per kernel (DESIGN.md "bytes per unit"), matching
 * the order of tpsrhs_kernel_times. */
int tpsrhs_kernel_bytes(tpsrhs_handle h, int capacity, const char **names, double *bytes);

/* ---- next row of the scope table: one explicit RK4 step on the device ----
 * Replaces M2ulPhyS::solveStep's `timeIntegrator->Step(*U, time, dt); Check_NAN(); Check_Undershoot();`
 * (src/M2ulPhyS.cpp:2004-2008) for the RK4 integrator (time-integrator type 4, src/M2ulPhyS.cpp:721-739):
 * the four stages of MFEM's RK4Solver::Step [third party: MFEM >= 4.4, linalg/ode.cpp] with the stage
 * combinations fused into one streaming kernel per stage, the NaN census of Check_NAN
 * (src/M2ulPhyS.cpp:2463-2524) and, for USER_DEFINED fluids, the species clamp of Check_Undershoot
 * (:2526-2548) fused into the last one.  x: device vector, updated in place; *time += dt.
 * max_char_speed (may be NULL): value left by the last stage's Mult, which the reference turns into the
 * next dt (src/M2ulPhyS.cpp:2013-2016).  nan_count (may be NULL): number of NaN entries of the new x. */
int tpsrhs_rk4_step(tpsrhs_handle h, double *x, double *time, double dt, double *max_char_speed, int64_t *nan_count);

/* The time loop on the device: `num_steps` times M2ulPhyS::solveStep (src/M2ulPhyS.cpp:2004-2019) --
 *   timeIntegrator->Step(*U, time, dt); Check_NAN(); Check_Undershoot();
 *   if (!constant_dt) dt = MPI_MIN over ranks of CFL * hmin / max_char_speed / dim;
 * -- with dt, the time and the NaN census kept in device memory, so that nothing returns to the host between
 * steps (one synchronisation at the end).  x: device vector, updated in place; *time and *dt: in/out (dt of
 * the NEXT step on return); hmin: the reference's minimum element size (mesh->GetElementSize(i, 1),
 * src/M2ulPhyS.cpp:757-761 [third party: MFEM], passed in by the adapter); nan_count (may be NULL): NaN entries
 * seen by the censuses of all steps (the reference exits at the first). */
int tpsrhs_advance(tpsrhs_handle h, double *x, double *time, double *dt, int num_steps, int constant_dt, double cfl,
                   double hmin, int64_t *nan_count);

/* The reference's other explicit integrators: `time/integrator` selects one of five (src/M2ulPhyS.cpp:2722-2736) and
 * the constructor builds MFEM's ForwardEulerSolver, RK2Solver(1.0), RK3SSPSolver, RK4Solver or RK6Solver from it
 * (src/M2ulPhyS.cpp:721-739) [third party: MFEM >= 4.4, linalg/ode.cpp].  The values are the reference's
 * timeIntegratorType.  In MFEM's order of operations, with k = f(.) one Mult:
 *   forward Euler   k = f(x);  x = x + dt*k
 *   RK2(a = 1)      k = f(x);  x1 = x + (dt/2)*k;  y = x + dt*k;  k = f(y);  x = x1 + (dt/2)*k
 *   RK3-SSP         k = f(x);  y = x + dt*k
 *                   k = f(y);  y = y + dt*k;  y = (3/4)*x + (1/4)*y
 *                   k = f(y);  y = y + dt*k;  x = (1/3)*x + (2/3)*y
 * Forward Euler, RK2 and RK3-SSP run the plain Mult followed by one streaming kernel per stage (each stage one pass
 * over the state: 3 / 7 / 11 state vectors of traffic per step); TPSRHS_RK4 is tpsrhs_rk4_step / tpsrhs_advance
 * themselves, bit for bit.  TPSRHS_RK6 (MFEM's eight-stage Verner scheme, which no input of the reference selects)
 * returns TPSRHS_ERR_UNSUPPORTED, any other value TPSRHS_ERR_INVALID_ARGUMENT, both before any device work. */
enum tpsrhs_integrator { TPSRHS_FORWARD_EULER = 1, TPSRHS_RK2 = 2, TPSRHS_RK3_SSP = 3, TPSRHS_RK4 = 4, TPSRHS_RK6 = 6 };

/* tpsrhs_rk4_step for any built integrator, argument for argument: x updated in place, *time += dt, max_char_speed
 * the value left by the LAST Mult of the step, Check_NAN and then (USER_DEFINED fluids) Check_Undershoot applied
 * once, to the final state of the step (src/M2ulPhyS.cpp:2004-2008).  The non-reflecting boundary state advances by
 * dt in every Mult, as in the reference: once per Euler step, twice per RK2 step, three times per RK3 step. */
int tpsrhs_step(tpsrhs_handle h, int integrator, double *x, double *time, double dt, double *max_char_speed,
                int64_t *nan_count);

/* tpsrhs_advance for any built integrator, argument for argument (the variable step, its MIN reduce hook, the
 * captured step graph, the read-back at the end are shared; a graph captured for one scheme is never replayed for
 * another). */
int tpsrhs_advance_with(tpsrhs_handle h, int integrator, double *x, double *time, double *dt, int num_steps,
                        int constant_dt, double cfl, double hmin, int64_t *nan_count);

/* ---- running statistics sampled in the time loop -------------------------------------------------------------------
 * What the reference's time loop does once per iteration besides solveStep: `average->addSample(iter, d_mixture)`
 * (src/M2ulPhyS.cpp:2099; src/averaging.cpp:198-234 the sampling condition and the counters, :331-435 the update) -- the
 * running mean of the primitive state and the running velocity covariances (the "rms" field), which the reference stores
 * as /meanSolution and /rmsData.
 *   mean[num_equation][NDofs]  in the layout of x and of tpsrhs_get_primitives (byNODES)
 *   vari[nvar][NDofs]          nvar = nvel (nvel + 1) / 2: the diagonal first, then the pairs i < j in row-major order --
 *                              uu vv ww uv uw vw for three velocity components, uu vv uv for two (src/M2ulPhyS.cpp:665-675)
 *   ns_mean, ns_vari           samples in each (apart, because restartRMS zeroes one and not the other)
 *   iter                       the step counter of the loop
 * One sample of a state x: s = prim(x) with the temperature row 1 + nvel replaced by the pressure; for every row
 * mean = (ns_mean mean + s) / (ns_mean + 1); then, with the UPDATED mean and d_i = s_i - mean_i of the velocity rows,
 * vari = (vari ns_vari + d_i d_j) / (ns_vari + 1); then both counters go up by one.  A field whose counter is 0 counts
 * as zero.  This is the reference's recurrence, not the textbook variance: two samples a, b give (b - a)^2 / 8.
 * Inside tpsrhs_advance / tpsrhs_advance_with, after every step: iter += 1, and if iter % sample_interval == 0 and
 * iter >= start_iter (the reference's sampleFreq and startIter) one sample of the new x is enqueued between the steps;
 * nothing returns to the host, the captured step graph is neither part of it nor re-captured because of it.
 * tpsrhs_step and tpsrhs_rk4_step neither count nor sample: a caller that drives the loop itself calls
 * tpsrhs_stats_add_sample.  Partitioned meshes need nothing more: the update is local to a node.
 * Two deliberate differences from the reference:
 *  (a) it samples the grid function Up, which holds the primitives of the input of the step's LAST Mult (a stage
 *      state); here the primitives of the new x are sampled, after Check_NAN and Check_Undershoot, whatever the integrator;
 *  (b) it replaces row 1 + dim by the pressure, which in the axisymmetric formulation (dim 2, three velocity
 *      components) is the swirl velocity; here it is the temperature row 1 + nvel in every formulation.
 * Every entry but tpsrhs_stats_configure returns TPSRHS_ERR_INVALID_ARGUMENT, before any device work, on an operator
 * whose statistics are not configured.  All pointers to fields are DEVICE pointers; the copies are ordered on the
 * operator's stream and do not synchronise (as tpsrhs_get_primitives). */

/* Allocates the fields (zero) and zeroes the counters and iter; compute_variances = 0: the mean only.  sample_interval
 * 0 switches statistics off and frees everything; a negative interval or start: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_stats_configure(tpsrhs_handle h, int64_t sample_interval, int64_t start_iter, int compute_variances);
/* The step counter the loop continues from (`iter` of a restart file). */
int tpsrhs_stats_set_iter(tpsrhs_handle h, int64_t iter);
/* One unconditional sample of the device vector x (iter is not touched). */
int tpsrhs_stats_add_sample(tpsrhs_handle h, const double *x);
/* Any pointer may be NULL. */
int tpsrhs_stats_get(tpsrhs_handle h, double *mean_out, double *vari_out, int *ns_mean, int *ns_vari, int64_t *iter);
/* Continuation (the reference's enableContinuation: samplesMean / samplesRMS and the two fields of a restart file).
 * vari == NULL or ns_vari == 0 is restartRMS: the covariances start again, the mean goes on.  ns_mean == 0 starts
 * the mean again too (mean may then be NULL). */
int tpsrhs_stats_set(tpsrhs_handle h, const double *mean, const double *vari, int ns_mean, int ns_vari);
/* nvar, or 0 when only the mean is kept */
int tpsrhs_stats_num_variances(tpsrhs_handle h, int *num_variances);

/* ---- fields at arbitrary points: planes and probes ------------------------------------------------------------------
 * What the reference's time loop does with the fields besides advancing and averaging them: it reads them where the user
 * wants them.  `planeDump` (src/M2ulPhyS.cpp:2052-2096, options :2812-2831) interpolates the conserved state, the
 * primitives, the mean or the Reynolds stresses onto an n x n plane through gslib's FindPointsGSLIB
 * (src/gslib_interpolator.cpp:53-84) [third party: gslib, optional; without it the reference prints an error].  Here the
 * operation is defined by the conventions at the top of this file and by nothing else:
 *   - the nodal tensor Lagrange basis on the p + 1 Gauss-Legendre or Gauss-Lobatto nodes of [0,1] (tpsrhs_disc::basis_type),
 *     l_a(t) = prod_{j != a} (t - x_j) / (x_a - x_j);  local = i + j*(p+1) + k*(p+1)^2;
 *   - order-1 geometry: element e maps the reference cube [0,1]^dim to space by the bi-/trilinear map through its
 *     elem_coords, MFEM vertex order (v0 at xi = 0; quad ccw; hex bottom ccw then top ccw).
 * A point is LOCATED in an element when Newton's iteration on that map, started at the element centre (at most 50
 * iterations), converges to reference coordinates that all lie in [-tol, 1 + tol]; they are not clamped.  A DG field has
 * two values on a face: among the elements that accept a point the one with the LOWEST INDEX answers.  This is part of
 * the contract.  A point no element accepts is "not found": element -1, reference coordinates 0, and `fill` as its value.
 * Point arrays use the reference's layout, xyz[i + d*npts] (src/gslib_interpolator.cpp:97-104); sampled values are
 * out[i + row*npts], the layout tpsrhs_eval_pointwise takes, so that sampled conserved states feed straight into it.
 * Axisymmetric runs are plain 2-D in (r, z).
 * Partitioned meshes: each rank locates, samples and records the points inside ITS OWN elements; elsewhere it reports
 * "not found".  A point on a face shared by two ranks may be found by both.  Combining the ranks (the reference's gslib
 * does it with its own MPI exchange) is the caller's job. */

/* FindPointsGSLIB::Setup + FindPoints (src/gslib_interpolator.cpp:53-67).  Host only, touches no device (like
 * tpsrhs_face_tables).  Candidates come from a uniform bin grid over the element bounding boxes, not from a sweep over the
 * elements.  elem_out[npts]; ref_out[i + d*npts] in [0,1] (up to tol).  tol <= 0: 1e-10.  Both dim 2 and dim 3.
 * NULL arguments, npts < 0, another dim: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_locate_points(const tpsrhs_mesh *mesh, int64_t npts, const double *xyz, double tol, int32_t *elem_out,
                         double *ref_out);
/* PlaneInterpolator::setInterpolationPoints (src/gslib_interpolator.cpp:121-190), point for point: the n x n lattice over
 * the bounding box [bb0, bb1] in the two directions other than the major direction of `normal` (the first of x, y, z with
 * the largest |component|), i fastest and j slowest, the third coordinate from normal . (x - point) = 0.
 * xyz_out: [3][n*n].  n < 2 or a NULL argument: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_plane_points(const double point[3], const double normal[3], const double bb0[3], const double bb1[3], int n,
                        double *xyz_out);

typedef struct tpsrhs_sampler *tpsrhs_sampler_handle;

/* FindPointsGSLIB::Setup + FindPoints on the operator's own (rank-local) mesh, order and basis (what
 * PlaneInterpolator::initializeFinder + setInterpolationPoints leave behind, src/gslib_interpolator.cpp:53-67): xyz is a
 * HOST array [dim][npts]; the element and reference coordinates of every point go to the device, sorted by element, with
 * the permutation back to the caller's order.  fill: the value of points that were not found (FindPointsGSLIB's default
 * is 0).  The operator OWNS its samplers: tpsrhs_destroy frees those that are left, and their handles die with it. */
int tpsrhs_sampler_create(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                          tpsrhs_sampler_handle *out);
/* Also switches the probes off when they record through this sampler.  NULL: nothing to do. */
int tpsrhs_sampler_destroy(tpsrhs_sampler_handle s);
/* FindPointsGSLIB::GetElem / GetReferencePosition / GetCode: HOST copies in the caller's order, elem_out[npts] (-1: not
 * found) and ref_out[i + d*npts]; nfound the number of located points.  Any output may be NULL. */
int tpsrhs_sampler_info(tpsrhs_sampler_handle s, int64_t *npts, int64_t *nfound, int32_t *elem_out, double *ref_out);
/* FindPointsGSLIB::Interpolate (src/gslib_interpolator.cpp:69-84; the four field choices of planeDump,
 * src/M2ulPhyS.cpp:2057-2087).  field: DEVICE, [nrows][NDofs], any byNODES array -- x, the output of tpsrhs_get_primitives,
 * the mean and vari of tpsrhs_stats_get; out: DEVICE, [nrows][npts] in the caller's point order; points that were not found
 * get `fill` in every row.  Asynchronous on the operator's stream.  nrows >= 1, no upper limit; a NULL argument or
 * nrows < 1: TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
int tpsrhs_sample(tpsrhs_sampler_handle s, int nrows, const double *field, double *out);

/* ---- point location on the device, and a field carried from one mesh to another ------------------------------------------
 * utils/pfield_interpolate.cpp:36-155 (a restart on another mesh or order) and CycleAvgJouleCoupling
 * (src/cycle_avg_joule_coupling.cpp:159-363, flow mesh <-> EM mesh at every coupling iteration) both form the physical
 * coordinates of the target's nodes, FindPointsGSLIB::Interpolate the source field there and SetFromTrueDofs the result.
 * Here the location rule is the one above, run with one lane per point (k_locate): the same bins, the same ascending walk,
 * the same Newton iteration and acceptance, from the same source text as the host locator.  The device contracts a*b + c
 * into an FMA where the host build does not, so reference coordinates differ from the host's in the last bits, and the
 * accepted element can differ ONLY for a point whose reference coordinate lies within rounding of -tol or 1 + tol -- a
 * point 1e-10 outside an element, not a point on a face. */

/* tpsrhs_sampler_create with the points already on the device and nothing returning to the host:
 * xyz DEVICE [dim][npts].  The points keep the caller's order (no sort: identity permutation) --
 * meant for point sets that are spatially coherent already, such as the nodes of another mesh.  The search grid of the
 * operator's mesh is uploaded once per (operator, tol) and freed by tpsrhs_destroy.  tpsrhs_sampler_info copies elem and
 * ref from the device on demand; tpsrhs_sample and the probes take such a sampler as any other.  Asynchronous on the
 * operator's stream (xyz must stay valid until that work has run); a NULL handle or output, npts < 0, NULL points with
 * npts > 0 or a NaN tol: TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
int tpsrhs_sampler_create_device(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                                 tpsrhs_sampler_handle *out);

/* Physical coordinates of the operator's DG nodes, DEVICE out[dim][NDofs], from the order-1 vertex map at
 * the operator's 1-D nodes (what pfield_interpolate.cpp:114-135 builds with ElementTransformation::Transform).
 * Asynchronous on the operator's stream.  A NULL argument: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_node_coordinates(tpsrhs_handle h, double *xyz_out);

/* pfield_interpolate.cpp:138-146 / CycleAvgJouleCoupling: field_dst[row][NDofs_dst] = field_src at the nodes of dst.
 * nrows rows of a byNODES field of src (x, primitives, means, visualization fields, a conductivity ...), DEVICE arrays.
 * Nodes of dst outside the mesh of src get `fill` in every row; *num_missing (may be NULL) is their count.
 * The first call for a pair creates a device sampler on src at dst's node coordinates and keeps it on src, keyed by dst
 * and tol (fill is taken at every call); it is dropped when either operator is destroyed.  Later calls are one k_sample
 * launch.  The work runs on src's stream and dst's stream waits for it through an event: no host synchronisation unless
 * num_missing is asked for (the locating first call of a pair synchronises once, to free the coordinates).  Orders, bases and element counts may differ freely; axisymmetric runs are plain 2-D in
 * (r, z); on partitioned meshes each rank transfers from its own elements (the sampler contract above).
 * NULL handle or array, nrows < 1, NaN tol, operators of different dim: TPSRHS_ERR_INVALID_ARGUMENT; operators on
 * different devices: TPSRHS_ERR_UNSUPPORTED -- both before any device work. */
int tpsrhs_transfer(tpsrhs_handle src, tpsrhs_handle dst, int nrows, const double *field_src, double *field_dst,
                    double tol, double fill, int64_t *num_missing);
/* Diagnostics of the pair cache: how many tpsrhs_transfer calls on src created a sampler (ran k_locate) and how many found
 * theirs.  Either output may be NULL. */
int tpsrhs_transfer_stats(tpsrhs_handle src, int64_t *num_located, int64_t *num_cache_hits);

/* Probe time histories inside the device time loop (the per-iteration use of the interpolator: the reference calls its
 * plane dump from solveStep, src/M2ulPhyS.cpp:2052-2096, on the host).  After
 * every step of tpsrhs_advance / tpsrhs_advance_with a step counter goes up (tpsrhs_probe_configure zeroes it); when
 * count % interval == 0 one record is enqueued between the steps:
 *   values[record][num_equation][npts]  the conserved state x at the sampler's points (tpsrhs_sample of x)
 *   times[record]                       the time, copied from DEVICE memory (the variable-dt loop never has it on the host)
 *   iters[record]                       the count
 * Nothing returns to the host; the record is never part of the captured step graph and never causes a re-capture.  When
 * `capacity` records are held further records are dropped and counted: nothing is overwritten, nothing is written past the
 * end.  tpsrhs_step and tpsrhs_rk4_step neither count nor record, as with the statistics.
 * s == NULL or interval == 0 switches the probes off and frees the buffer; a negative value, capacity < 1 with probes on,
 * or a sampler of another operator: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_probe_configure(tpsrhs_handle h, tpsrhs_sampler_handle s, int64_t interval, int64_t capacity);
/* Copies the held records to HOST arrays (iters_out[nrecords], times_out[nrecords], values_out[nrecords][neq][npts]) and
 * synchronises the stream.  Any pointer may be NULL.  reset != 0 starts the buffer again (records and dropped count) and
 * leaves the step counter alone.  Probes not configured: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_probe_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                      double *values_out, int reset);

/* The time step the non-reflecting boundary conditions integrate their boundary state with: the reference's
 * BoundaryCondition holds a reference to M2ulPhyS::dt (src/BoundaryCondition.hpp:54) and advances `boundaryU`
 * by dt in EVERY Mult (src/outletBC.cpp:712-724).  tpsrhs_rk4_step sets it itself. */
int tpsrhs_set_dt(tpsrhs_handle h, double dt);

/* ---- fields on a refined element lattice: what a ParaView output step evaluates ------------------------------------------
 * The reference's time loop and its visualization mode end in paraviewColl->Save() (src/M2ulPhyS.cpp:443-446, 1877-1906,
 * 2043-2045, 4131-4133): a ParaViewDataCollection with SetLevelsOfDetail(order), for which MFEM evaluates every registered
 * grid function at a closed uniform lattice of each element (GridFunction::GetValues at the points of a RefinedGeometry).
 * The conventions are those of the sampling section above (basis, local numbering, order-1 geometry), and in addition:
 *   - for levels = L, 1 <= L <= TPSRHS_MAXLATTICE, every element carries the lattice t_a = a / L, a = 0..L, per direction;
 *     local = a + b*(L+1) + c*(L+1)^2; point index = e*(L+1)^dim + local; npts = num_elements*(L+1)^dim;
 *   - arrays are [row][npts];
 *   - a point on a face shared by two elements exists once PER ELEMENT and carries that element's own polynomial (the
 *     sampler lets the lowest-index element answer there; a DG picture needs both values).
 * The evaluation is a sum-factorised contraction of an element's nodal tile with the 1-D matrix B[a][i] = l_i(a / L)
 * (k_lattice, lattice.hpp): dim*(p+1) multiply-adds per value, the field read once, no location records.  B is formed on
 * the host in double at every call from the operator's own nodes; the entries keep no state on the operator.
 * All three are asynchronous on the operator's stream except tpsrhs_lattice_size, which touches no device.  A NULL
 * argument, nrows < 1 or levels outside 1..TPSRHS_MAXLATTICE: TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
#define TPSRHS_MAXLATTICE 8
/* points_per_element = (levels+1)^dim, npts = num_elements * points_per_element.  Host only. */
int tpsrhs_lattice_size(tpsrhs_handle h, int levels, int64_t *points_per_element, int64_t *npts);
/* xyz_out: DEVICE [dim][npts], the bi-/trilinear vertex map at the lattice points.  The shape weights are products of t
 * and 1 - t (as in tpsrhs_node_coordinates), so a lattice corner is the element's vertex bit for bit. */
int tpsrhs_lattice_coordinates(tpsrhs_handle h, int levels, double *xyz_out);
/* field: DEVICE [nrows][NDofs], any byNODES array; out: DEVICE [nrows][npts], doubles, or with out_float32 != 0 floats:
 * the double result converted once, round to nearest (ParaView files are normally single precision, and the copy to the
 * host is the expensive part of an output step).  nrows >= 1, no upper limit. */
int tpsrhs_lattice_fields(tpsrhs_handle h, int levels, int nrows, const double *field, void *out, int out_float32);

/* ---- next row of the scope table: the other ForcingTerms of RHSoperator ----
 * RHSoperator appends these to its `forcing` array (src/rhs_operator.cpp:101-166) and adds them to y
 * after the inverse mass (src/rhs_operator.cpp:451-461).  SourceTerm and AxisymmetricSource follow from
 * tpsrhs_physics / tpsrhs_disc; the ones below are configured here, after tpsrhs_create. */
#define TPSRHS_MAXHEATSOURCES 4
#define TPSRHS_MAXSPONGEZONES 2
#define TPSRHS_MAXPASSIVESCALARS 4

typedef struct tpsrhs_heat_source { /* heatSourceData, type "cylinder" (src/dataStructures.hpp:528-535) */
  double value;                      /* added to y[(dim+1)*NDofs + node] (src/forcing_terms.cpp:923-936) */
  double radius, point1[3], point2[3];
} tpsrhs_heat_source;

enum tpsrhs_sponge_type { TPSRHS_SPONGE_PLANAR = 0, TPSRHS_SPONGE_ANNULUS = 1 };  /* SpongeZoneType */
enum tpsrhs_sponge_solution { TPSRHS_SPONGE_USERDEF = 0, TPSRHS_SPONGE_MIXEDOUT = 1 }; /* SpongeZoneSolution */

typedef struct tpsrhs_sponge_zone { /* SpongeZoneData (src/dataStructures.hpp:260-287) */
  int type;                          /* tpsrhs_sponge_type */
  int solution_type;                 /* tpsrhs_sponge_solution.  MIXEDOUT (src/forcing_terms.cpp:713-743): at every
                                      * Mult the target is the mixed-out state of the mean convective normal flux over
                                      * the nodes within `tol` of the plane through point_init (planar zone) / of the
                                      * cylinder of radius r1 (annulus), summed over the ranks with runtime.reduce;
                                      * target_U is ignored.  Dry air, planar 2-D / 3-D; else TPSRHS_ERR_UNSUPPORTED */
  double tol;                        /* MIXEDOUT: node search tolerance (spongezone/tolerance) */
  double normal[3], point0[3], point_init[3]; /* normal is normalised by the library (forcing_terms.cpp:528-532) */
  double r1, r2;                     /* annulus radii */
  double mult_factor;
  /* SpongeZone::targetU, the CONSERVED target state the constructor derives from targetUp with the
   * mixture's modifyEnergyForPressure (src/forcing_terms.cpp:486-517); the adapter copies it from there.
   * Its speed of sound (forcing_terms.cpp:653-656) is evaluated by the library. */
  double target_U[TPSRHS_MAXEQUATIONS];
} tpsrhs_sponge_zone;

/* PassiveScalar ([passiveScalars], src/M2ulPhyS.cpp:2855-2875; src/forcing_terms.cpp:768-870): at the nodes closer than
 * `radius` to `coords` (the first `dim` entries), y[(num_equation-1) NDofs + node] -= |u| (Up_last - rho value) / radius
 * with |u| over the `dim` velocity components and Up_last the LAST primitive variable -- whatever the equation system
 * (the reference appends the term whenever such an entry exists: test/inputs/argonMinimal.ini:118-124 relaxes the last
 * species of the ternary plasma with it). */
typedef struct tpsrhs_passive_scalar { /* passiveScalarData (src/dataStructures.hpp:519-526) */
  double coords[3];
  double radius;
  double value;
} tpsrhs_passive_scalar;

typedef struct tpsrhs_forcing {
  int has_pressure_gradient;         /* config.thereIsForcing(): ConstantPressureGradient, forcing_terms.cpp:115-171 */
  double pressure_gradient[3];
  int num_heat_sources;              /* enabled HeatSource entries only */
  tpsrhs_heat_source heat_sources[TPSRHS_MAXHEATSOURCES];
  int num_sponge_zones;              /* SpongeZone */
  tpsrhs_sponge_zone sponge_zones[TPSRHS_MAXSPONGEZONES];
  int num_passive_scalars;           /* PassiveScalar */
  tpsrhs_passive_scalar passive_scalars[TPSRHS_MAXPASSIVESCALARS];
} tpsrhs_forcing;

/* Replaces the forcing.Append(...) calls of the RHSoperator constructor for ConstantPressureGradient, PassiveScalar,
 * SpongeZone and HeatSource.  NULL removes them. */
int tpsrhs_set_forcing(tpsrhs_handle h, const tpsrhs_forcing *forcing);

/* MixingLengthTransport (src/mixing_length_transport.cpp:44-131; [flow] useMixingLength, flow/mixing-length/...,
 * src/M2ulPhyS.cpp:265-277, 2701-2708): an algebraic eddy viscosity rho l^2 |S| with l = min(0.41 d, max_mixing_length)
 * on top of the molecular transport of the flux (viscosity, bulk viscosity, heavy-species conductivity; not the
 * species diffusivities, not the source terms), d = the wall-distance grid function `distance_` of the reference:
 * `distance` is its DEVICE array (NDofs doubles, owned by the caller, read at every Mult).  NULL switches the model off.
 * Built for the 2-D kernels (planar and axisymmetric mixtures, axisymmetric dry air: the formulations of the reference's
 * inputs that use it, test/inputs/plasma.ini:48, pipe.axisym.mix.ini:19); 3-D and planar dry air:
 * TPSRHS_ERR_UNSUPPORTED. */
typedef struct tpsrhs_mixing_length { /* mixingLengthTransportData (src/dataStructures.hpp:548-554) */
  double max_mixing_length; /* 0 turns the model off, as in the reference */
  double pr_ratio;          /* flow/mixing-length/Pr_ratio (`Prt_`), default 1 */
  double lewis;             /* `Let_`: read by the reference, not used by its flux transport */
  double bulk_multiplier;   /* bulk eddy viscosity = bulk_multiplier * mu_t */
} tpsrhs_mixing_length;
int tpsrhs_set_mixing_length(tpsrhs_handle h, const double *distance, const tpsrhs_mixing_length *params);

/* ---- the wall-distance function (flow/computeDistance) -----------------------------------------------------------------
 * What the reference computes once at start-up when `flow/computeDistance` is set (src/M2ulPhyS.cpp:371-437, every input
 * with useMixingLength sets it): the distance from every DG node to the nearest wall boundary face,
 * evaluateDistanceSerial (src/utils.cpp:371-514) -- there one serial host loop over nodes x wall faces; here the faces are
 * selected on the host (tpsrhs_wall_faces) and the all-pairs search runs on the device (tpsrhs_wall_distance).  The result
 * is the `distance` array tpsrhs_set_mixing_length takes.  The operation, defined by the conventions at the top of this file:
 *   - the node coordinates xp are those of the DG nodes under the order-1 geometry: the bi-/trilinear map through
 *     elem_coords at the tensor Gauss-Legendre / Gauss-Lobatto nodes of the operator (the reference's `coordinates` grid
 *     function after SetCurvature(1)).  Axisymmetric runs are plain 2-D in (r, z).
 *   - a wall face is the straight segment (2-D) or the bilinear quadrilateral (3-D) through its 2 / 4 corners, X(xi) on
 *     [0,1]^(dim-1); corner = ta + 2 tb.
 *   - per (node, face): start at the centre xi = 1/2; dx = xp - X(xi), res = -J^T dx with J = dX/dxi (dim x (dim-1)),
 *     r0 = |res|; while (|res| > 1e-16 && |res| / r0 > 1e-10 && iter < 20): xi += (J^T J)^{-1} J^T dx (the Hessian of the
 *     map is neglected, as in the reference) and dx, res are formed again; with r0 == 0 the loop is skipped.  Then every
 *     coordinate of xi is clamped to [0,1] [third party: MFEM Geometry::CheckPoint / ProjectPoint for SEGMENT and SQUARE]
 *     and the distance to the face is |xp - X(xi)|.
 *   - distance[node] = the minimum over the faces, kept with `<`, starting from 1e30: without a wall face every entry is
 *     1e30, and a NaN distance (a collapsed face) never wins.
 * The orientation of a face does not matter (the iteration and the clamp are invariant under the symmetries of the
 * reference square).  The reference prints a warning when the iteration stops at its cap; NOTHING corresponds to it here,
 * on purpose: for affine faces Newton lands in one step and the warning then fires whenever r0 itself is at rounding
 * level, so its count is rounding noise and no part of a contract.  Curved (order > 1) geometry is not built. */

/* Host only, touches no device (like tpsrhs_face_tables and tpsrhs_locate_points): the corner coordinates of the wall
 * boundary faces of `mesh`.  num_attributes >= 0: the boundary faces whose attribute is in `attributes` (bcs may be
 * NULL).  num_attributes < 0: the reference's rule (src/M2ulPhyS.cpp:392-398) -- every entry of `bcs` of category
 * TPSRHS_WALL whose type is not TPSRHS_INV.  face_xyz_out[face][corner][dim], corner = ta + 2 tb of the owning element's
 * local face (2^(dim-1) corners), coordinates from the owning element's elem_coords (periodic meshes keep their geometry);
 * faces in ascending (element, local face) order.  *num_faces_out is always the full count; min(count, capacity) faces are
 * written, and face_xyz_out may be NULL with capacity == 0.  A boundary record that matches no element face, a NULL mesh,
 * a dim other than 2 / 3, a negative capacity or a missing array: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_wall_faces(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int num_attributes, const int *attributes,
                      int64_t capacity, double *face_xyz_out, int64_t *num_faces_out);

/* distance_out[NDofs] (DEVICE) = the wall distance of every node of the operator to the num_faces faces of face_xyz (HOST,
 * the layout of tpsrhs_wall_faces, dim = the operator's).  Ordered on the operator's stream, which is synchronised before
 * the call returns (a start-up function: its temporary face table on the device is freed then); every entry of
 * distance_out is written, also for num_faces == 0 (1e30).  Divisions and square roots are IEEE (correctly rounded).
 * Partitioned meshes: a rank's nodes need the wall faces of ALL ranks (the reference computes on the serial mesh): every
 * rank calls tpsrhs_wall_faces on its own mesh and the caller concatenates the lists (an all-gather) -- the caller's job,
 * as with the samplers.  num_faces < 0, a NULL handle or output, NULL faces with num_faces > 0 or a face coordinate that is
 * not finite: TPSRHS_ERR_INVALID_ARGUMENT before any device work.  TPSRHS_WALLDIST_CULL=0 (environment, read per call)
 * switches off the conservative cull -- a face whose bounding sphere lies farther from the node than the best distance so
 * far cannot win the minimum and is skipped; the results are bit-equal either way. */
int tpsrhs_wall_distance(tpsrhs_handle h, int64_t num_faces, const double *face_xyz, double *distance_out);

/* ---- volume integrals, L2 errors, extrema and the monitor history of the time loop ------------------------------------
 * The global numbers a solver's time loop reports: the conserved totals, the range of every state variable, the L2 error
 * against a known solution -- M2ulPhyS::checkSolutionError (src/masa_handler.cpp:139-152) through
 * GridFunction::ComputeLpError(2, ...) [third party: MFEM, fem/gridfunc.cpp; its default rule is Gauss-Legendre of order
 * 2p + 3] -- the mean |dU/dt| per equation (RHSoperator::computeMeanTimeDerivatives, src/rhs_operator.cpp:833-849) and the
 * step-size history, which with a variable step exists only in device memory.  All are reductions over a byNODES field.
 * THE RULE, part of the contract:
 *   - tensor Gauss-Legendre with NQ = p + 2 points per direction on [0,1] (MFEM's order 2p + 3), points numbered
 *     q = e*NQ^dim + (i + j*NQ + k*NQ^2);
 *   - order-1 geometry, as for the samplers: the bi-/trilinear map through elem_coords;
 *   - W_q = w_i w_j (w_k) |det J(xi_q)|, and with radial_weight != 0  W_q r_q, r_q the FIRST coordinate of the mapped
 *     point (the axisymmetric formulation's (r, z)); there is no factor 2 pi;
 *   - a nodal field is evaluated at the points with the operator's Lagrange basis (Gauss-Legendre or Gauss-Lobatto
 *     nodes), one direction after the other (sum factorisation).
 * The rule is exact for f_h, for f_h^2 and for both times det J of a trilinear hexahedron (degree <= 2p + 2 per direction).
 * SUMMATION STRUCTURE, part of the contract: the terms of one element are summed first, the element sums are combined in
 * a fixed order, and a last single-block kernel reads the per-block partials.  No floating-point atomics: two calls on
 * the same input give the same bits.  With K = NQ^dim + ne + 8 dim (p+1) the rounding error of `sum` is at most
 * K eps sum_q W_q A_q and that of `sumsq` at most 2 K eps sum_q W_q (A_q + |exact_q|)^2, A_q = sum_n |l_n(xi_q)| |f_n|.
 * Partitioned meshes: every rank reduces its own elements and the caller combines the ranks, as with the samplers. */

/* Host only, touches no device: the points and weights of the rule on `mesh` for polynomial order `order`.
 * xyz_out[d*npts + q] (the layout of tpsrhs_locate_points), w_out[q] = W_q WITHOUT the radial factor; either may be NULL;
 * *npts_out = num_elements * NQ^dim is always written.  A NULL mesh or npts_out, a dim other than 2 / 3 or an order outside
 * 1 ... TPSRHS_MAXORDER: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_quadrature_points(const tpsrhs_mesh *mesh, int order, double *xyz_out, double *w_out, int64_t *npts_out);

/* g_q = f_h(xi_q) - exact_q[row][q] (exact_q == NULL counts as 0):  sum_out[row] = sum_q W_q g_q,
 * sumsq_out[row] = sum_q W_q g_q^2 -- sqrt(sumsq) is ComputeLpError(2, .).  field: DEVICE [nrows][NDofs], any byNODES
 * array; exact_q: DEVICE [nrows][npts] at the points of tpsrhs_quadrature_points, or NULL; the outputs: DEVICE [nrows],
 * either may be NULL.  Asynchronous on the operator's stream; the field is read once.  nrows >= 1, no upper limit; a NULL
 * handle or field, or nrows < 1: TPSRHS_ERR_INVALID_ARGUMENT before any device work.  The scratch belongs to the operator
 * (allocated at the first call, freed by tpsrhs_destroy). */
int tpsrhs_integrate(tpsrhs_handle h, int nrows, const double *field, const double *exact_q, int radial_weight,
                     double *sum_out, double *sumsq_out);

/* Per row of field (DEVICE [nrows][NDofs]): min_out, max_out and meanabs_out = sum_n |f_n| / NDofs (DEVICE [nrows], each
 * may be NULL) -- computeMeanTimeDerivatives for field = y = Mult(x).  min and max start from +-inf and are kept with
 * `<` / `>`: a NaN entry never wins (as in the wall distance); a NaN does propagate into meanabs.  Same summation
 * structure, stream and refusals as tpsrhs_integrate. */
int tpsrhs_nodal_stats(tpsrhs_handle h, int nrows, const double *field, double *min_out, double *max_out,
                       double *meanabs_out);

/* Monitor history inside the device time loop.  After every step of tpsrhs_advance / tpsrhs_advance_with a step counter
 * goes up (tpsrhs_monitor_configure zeroes it); when count % interval == 0 one record is enqueued between the steps:
 *   iters[record]              the count
 *   times[record], dts[record] the time and the dt of the NEXT step, copied device-to-device from the loop's control block
 *   totals[record][neq]        tpsrhs_integrate of the new x, radial_weight = the operator's axisymmetric flag
 *   mins, maxs[record][neq]    tpsrhs_nodal_stats of x
 * The semantics of the probes: nothing returns to the host, a record is never part of the captured step graph and never
 * causes a re-capture; when `capacity` records are held further records are dropped and counted, and nothing is written
 * past the end; tpsrhs_step and tpsrhs_rk4_step neither count nor record.  interval == 0 switches the monitor off and
 * frees its buffers; a negative value, or capacity < 1 with the monitor on: TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_monitor_configure(tpsrhs_handle h, int64_t interval, int64_t capacity);
/* Copies the held records to HOST arrays and synchronises the stream.  Any pointer may be NULL.  reset != 0 starts the
 * buffer again (records and dropped count) and leaves the step counter alone.  Monitor not configured:
 * TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_monitor_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                        double *dts_out, double *totals_out, double *mins_out, double *maxs_out, int reset);

/* ---- surface integrals over boundary patches, and their history in the time loop --------------------------------------
 * The reference integrates one thing over a boundary patch: its area, at start-up, for every inlet and outlet --
 * BoundaryCondition::aggregateArea / aggregateBndryFaces (src/BoundaryCondition.cpp:59-92), printed by
 * OutletBC::computeParallelArea (src/outletBC.cpp:329-343) and src/inletBC.cpp:306-307; the mass-flow outlets
 * (TPSRHS_SUB_MF_NR / _PW) need it in data[7].  Here the same reduction takes any byNODES array: the area is the integral
 * of ones, and the mass flow through a patch, the pressure and viscous force on a body and the heat load on a wall are
 * integrals of arrays this library already has on the device (tpsrhs_get_primitives, tpsrhs_get_gradients,
 * tpsrhs_eval_pointwise, tpsrhs_visualization_fields).  Those forces and loads are COMPOSITIONS THE REFERENCE DOES NOT
 * HAVE; nothing of it is restated by them.  The library knows no physics here: it integrates what the caller hands it.
 * The host selects the faces (tpsrhs_patch_faces, or any list of the caller's), the device computes.
 * A FACE is (element, local face), local face = 2 d + s: reference direction d, side xi_d = s -- the slot convention of
 * tpsrhs_face_tables.  Any element face may be in a set, also an interior one (a station plane inside the mesh).
 * THE RULE, part of the contract:
 *   - on face (d, s) the points are the tensor Gauss-Legendre points with NQ = p + 2 per tangential direction on
 *     [0,1]^(dim-1); the tangential directions a < b are the other reference directions in ascending order, xi_d = s,
 *     points numbered i + j*NQ (i along a);
 *   - order-1 geometry, as for the samplers and the volume integrals: the bi-/trilinear map X through elem_coords;
 *   - the area-weighted outward normal at a point is N_q = (2s - 1) sgn(det J) cof(J) e_d with cof(J) = det(J) J^{-T},
 *     J = dX/dxi at the point (2-D, d = 0: (dy/dxi_1, -dx/dxi_1)); it is the normal of the sweeps and a polynomial of
 *     degree <= 1 per tangential direction;
 *   - dS_q = w_i w_j |N_q| and n dS = w_i w_j N_q (no square root in FLUX and NORMAL); with radial_weight != 0 every
 *     weight is multiplied by r_q, the FIRST coordinate of the mapped point; there is no factor 2 pi;
 *   - a nodal field is evaluated at the points with the operator's Lagrange basis (Gauss-Legendre or Gauss-Lobatto
 *     nodes): the trace along d at xi_d = s first, then one tangential direction after the other.
 * FLUX and NORMAL are exact for every f_h on every bilinear face (degree p + 1 <= 2p + 3 per direction).  SCALAR is exact
 * on planar faces whose |N| is a polynomial (parallelograms, and planar faces in general up to the degree of the rule); on
 * a warped face |N_q| is not a polynomial and SCALAR is a quadrature of it, not an exact integral.
 * SUMMATION STRUCTURE, part of the contract: the terms of one face are summed first (a butterfly over its points).  The faces
 * of a patch, sorted by (element, local face), are cut into fixed runs that never cross a patch boundary; a run is walked
 * in batches of FB consecutive faces (FB = 64 / the power of two >= NQ^(dim-1)), and running sum k of the run collects the
 * face sums k, k + FB, k + 2 FB, ... of the run in ascending order.  A last single-block kernel adds the running sums of a
 * patch, taken in the order (run, k): lane t of one wave the entries t, t + 64, ... in ascending order, then a butterfly
 * over the 64 lanes.  The order depends on the sorted face list and the order p alone.  No floating-point atomics: two calls
 * on the same input give the same bits, and so do two surfaces made of the same faces in any input order.  With K_s = NQ^(dim-1) + nf_p + 8 dim (p+1) + 16, nf_p the faces of the
 * patch, the rounding error of an output is at most K_s eps sum_q w_q G_q R_q A_q over the points of the patch, where
 * G_q = |dX/da| |dX/db| (3-D; |dX/da| in 2-D) bounds |N_q|, R_q = |r_q| with the radial weight and 1 without, and
 * A_q = sum_n |l_n(xi_q)| |f_n| (summed over the dim components for FLUX).  The terms of K_s: the butterfly over a face's
 * points, the sums over the faces of the patch, the dim (p+1)-term interpolations with their products, and 16 for the
 * geometry (the map, the cofactors, the weight).
 * Partitioned meshes: every rank reduces its own faces and the caller combines the ranks, as with the volume integrals. */

/* Host only, touches no device (next to tpsrhs_wall_faces): the boundary faces of `mesh` whose attribute is attributes[p],
 * as elem_out, face_out (local face 2 d + s) and patch_out = p -- the faces aggregateBndryFaces
 * (src/BoundaryCondition.cpp:76-92) counts per patch.  Ascending (element, local face) order, a boundary record matched to
 * its owning element as tpsrhs_wall_faces matches it.  *num_faces_out is always the full count; min(count, capacity) faces
 * are written, and the arrays may be NULL with capacity == 0.  An attribute without a face on this mesh gives an empty
 * patch (on a partitioned mesh some ranks have none).  An attribute listed twice, num_attributes < 1, a boundary record
 * that matches no element face, a NULL mesh, a dim other than 2 / 3, a negative capacity or a missing array:
 * TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_patch_faces(const tpsrhs_mesh *mesh, int num_attributes, const int *attributes, int64_t capacity,
                       int32_t *elem_out, int32_t *face_out, int32_t *patch_out, int64_t *num_faces_out);

typedef struct tpsrhs_surface_s *tpsrhs_surface_handle;
/* A set of num_faces faces in num_patches patches on the operator's mesh: what a BoundaryCondition of the reference holds
 * of its patch once aggregateBndryFaces has run (src/BoundaryCondition.cpp:76-92: the faces of the attribute, their count),
 * kept for the integrals instead of one number.  elem, face, patch: HOST arrays [num_faces]; the
 * library sorts them by (patch, element, face) and keeps them on the device.  num_faces == 0 is legal (elem, face, patch
 * may then be NULL): every integral of it is zero; so is a patch without faces.  A duplicate (element, face), an element
 * outside 0 .. ne-1, a face outside 0 .. 2 dim - 1, a patch outside 0 .. num_patches-1, num_patches < 1, num_faces < 0 or
 * a NULL handle / out: TPSRHS_ERR_INVALID_ARGUMENT before any device work.  The surface belongs to its operator, as a
 * sampler does: tpsrhs_destroy frees the surfaces that are still alive, and their handles are dead afterwards. */
int tpsrhs_surface_create(tpsrhs_handle h, int num_patches, int64_t num_faces, const int32_t *elem, const int32_t *face,
                          const int32_t *patch, tpsrhs_surface_handle *out);
/* No counterpart in the reference: what aggregateArea / aggregateBndryFaces fill (src/BoundaryCondition.cpp:59-92) lives
 * as long as its BoundaryCondition; here the set can go before its operator.  NULL is a
 * no-op.  A surface the patch history holds (tpsrhs_surface_monitor_configure) switches the history off first, records
 * included -- the rule of tpsrhs_sampler_destroy for the sampler of the probes.  A handle that is no live surface -- destroyed
 * already, or its operator destroyed -- is TPSRHS_ERR_INVALID_ARGUMENT here and in _info, _integrate and
 * _monitor_configure: the library keeps a list of the live surfaces and reads nothing of a handle that is not on it. */
int tpsrhs_surface_destroy(tpsrhs_surface_handle s);
/* Any pointer may be NULL.  faces_per_patch[num_patches]: what aggregateBndryFaces counts (src/BoundaryCondition.cpp:76-92). */
int tpsrhs_surface_info(tpsrhs_surface_handle s, int *num_patches, int64_t *num_faces, int64_t *faces_per_patch);
enum tpsrhs_surface_form { TPSRHS_SURFACE_SCALAR = 0, TPSRHS_SURFACE_FLUX = 1, TPSRHS_SURFACE_NORMAL = 2 };
/* field, out: DEVICE.  The value (row r, component c, node) is field[r*row_stride + c*comp_stride + node]; comp_stride is
 * read by FLUX only.  Per patch p:
 *   SCALAR  out[p*nrows + r]           = int f_r dS        (f = 1: aggregateArea, src/BoundaryCondition.cpp:59-74,
 *                                                            the number computeParallelArea prints, src/outletBC.cpp:329-343)
 *   FLUX    out[p*nrows + r]           = int F_r . n dS    F_r with dim components
 *   NORMAL  out[(p*nrows + r)*dim + k] = int f_r n_k dS
 * With row_stride = NDofs the arrays of tpsrhs_mult ([eq][NDofs]) go in as they are, and with row_stride = NDofs,
 * comp_stride = neq*NDofs those of tpsrhs_get_gradients ([d][eq][NDofs]).  Asynchronous on the operator's stream; the
 * field is read once; the scratch belongs to the surface.  nrows >= 1, no upper limit (rows are processed in passes).  A
 * NULL surface, field or output, nrows < 1 or an unknown form: TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
int tpsrhs_surface_integrate(tpsrhs_surface_handle s, int form, int nrows, const double *field, int64_t row_stride,
                             int64_t comp_stride, int radial_weight, double *out);

/* Patch history inside the device time loop, the fourth observer beside statistics, probes and monitor: the history of
 * what computeParallelArea (src/outletBC.cpp:329-343) computes once.  After every step of tpsrhs_advance /
 * tpsrhs_advance_with a step counter goes up (this call zeroes it); when count % interval == 0 one record is enqueued
 * between the steps:
 *   iters[record]                      the count
 *   times[record]                      the time, copied device-to-device from the loop's control block
 *   integrals[record][patch][neq]      SCALAR of the rows of the new x
 *   mass_flow[record][patch]           FLUX of the momentum rows 1 .. dim of x (comp_stride = NDofs)
 * both with radial_weight = the operator's axisymmetric flag.  The semantics of tpsrhs_probe_configure and
 * tpsrhs_monitor_configure: nothing returns to the host, a record is never part of the captured step graph and never
 * causes a re-capture; when `capacity` records are held further records are dropped and counted, and nothing is written
 * past the end; tpsrhs_step and tpsrhs_rk4_step neither count nor record.  s == NULL or interval == 0 switches the history
 * off and frees its buffers; a surface of another operator, a negative interval, or capacity < 1 with the history on:
 * TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_surface_monitor_configure(tpsrhs_handle h, tpsrhs_surface_handle s, int64_t interval, int64_t capacity);
/* Copies the held records to HOST arrays and synchronises the stream.  Any pointer may be NULL.  reset != 0 starts the
 * buffer again (records and dropped count) and leaves the step counter alone.  History not configured:
 * TPSRHS_ERR_INVALID_ARGUMENT. */
int tpsrhs_surface_monitor_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                                double *integrals_out, double *mass_flow_out, int reset);

/* ---- the nodal flux tensor of RHSoperator::GetFlux (src/rhs_operator.cpp:493-559) and the loads on a patch ---------------
 * The third array RHSoperator::Mult works from, beside the primitives and their gradients: per node
 *   CONVECTIVE  Fluxes::ComputeConvectiveFluxes(state)                              src/fluxes.cpp:135-170
 *   VISCOUS     Fluxes::ComputeViscousFluxes(state, gradUp, xyz, delta, dist)       src/fluxes.cpp:178-335, with ITS sign;
 *               zero for TPSRHS_EULER
 *   TOTAL       CONVECTIVE - VISCOUS, the flux(i, d, k) of GetFlux (:532-541)
 * x, out: DEVICE.  out[d][eq][node], dim * neq * NDofs doubles: the layout of tpsrhs_get_gradients, so it goes into
 * tpsrhs_surface_integrate(FLUX) with row_stride = NDofs, comp_stride = neq*NDofs and into tpsrhs_sample as it is.  In the
 * axisymmetric formulation dim = 2 and the rows include the swirl momentum, as in GetFlux.
 * The state is x with the species rows clamped at zero (:512-517); gradUp is the operator's; xyz is the node's position on
 * the order-1 map; delta is elSize (:154); dist is the distance array of tpsrhs_set_mixing_length when one is set; the
 * radius goes to the axisymmetric and table-gas closures: every closure gets the context the flux sweep of tpsrhs_mult
 * gives it, sub-grid scale models, viscous sponge and mixing length included.
 * gradients_current == 0: the call first runs what tpsrhs_update_gradients(h, x) runs (as tpsrhs_visualization_fields
 * does), then the pass.  gradients_current != 0: the caller asserts that Up / gradUp of x are held (after tpsrhs_mult(x)
 * or tpsrhs_update_gradients(x)); the pass alone runs.
 * NUMERICAL RULES, part of the contract: VISCOUS is evaluated from the closure's own terms, never as a difference of the
 * other two (on a wall F_v is many orders below F_c); TOTAL is formed from the two parts by ONE subtraction per entry.
 * The eight Coulomb collision fits of the argon-minimal transport are evaluated from their FORMULAS here; the flux sweep of
 * the 3-D p = 3 ternary kernels reads them from a polynomial table, so TOTAL differs from what that
 * sweep contracts by the table's documented error (tps_amd/csrc/coulomb_table.hpp: rounding of one Horner chain per fit,
 * measured by tests/test_coulomb_table.py) -- and is comparable with the CPU oracle.
 * Asynchronous on the operator's stream.  The pass reads nothing but x, gradUp and the mesh and writes nothing but out: a
 * later tpsrhs_mult gives the bits it would have given.  Every gas model, formulation, basis pair and order an operator
 * exists for is served.  NULL h, x or out, or an unknown part: TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
enum tpsrhs_flux_part { TPSRHS_FLUX_TOTAL = 0, TPSRHS_FLUX_CONVECTIVE = 1, TPSRHS_FLUX_VISCOUS = 2 };
int tpsrhs_get_flux(tpsrhs_handle h, const double *x, int part, int gradients_current, double *out);
/* out[patch][neq] (DEVICE) = int F_part . n dS per patch: tpsrhs_get_flux into a scratch of dim*neq*NDofs doubles that
 * belongs to the surface (allocated at the first call, freed with the surface), then the FLUX reduction of
 * tpsrhs_surface_integrate with radial_weight = the operator's axisymmetric flag -- its rule, summation structure, error
 * bound and determinism.  A COMPOSITION THE REFERENCE DOES NOT HAVE.  n points out of the element: on a wall patch the
 * momentum rows of TOTAL are the force the fluid exerts on the wall, pressure and viscous, and the energy row is the power
 * leaving the fluid through the patch (VISCOUS alone: minus the viscous force, minus the conducted and diffused power).
 * F is the flux of the INTERIOR trace extrapolated with the operator's basis, NOT the numerical boundary flux of the
 * boundary-condition classes; the two agree to the order of the scheme.  Partitioned meshes: each rank reduces its own
 * faces and the caller adds.  A handle that is no live surface, a NULL x or out, an unknown part:
 * TPSRHS_ERR_INVALID_ARGUMENT before any device work. */
int tpsrhs_surface_loads(tpsrhs_surface_handle s, const double *x, int part, int gradients_current, double *out);

/* ---- plasma post-processing fields: M2ulPhyS::updateVisualizationVariables (src/M2ulPhyS.cpp:4156-4263, the fields it
 * registers at :1690-1787), which the reference has on the CPU only (its device build exits at :4157-4160) -------------
 * One DEVICE array out[nrows][NDofs], the rows in the reference's registration order (names as it writes them):
 *   X_<sp>, Y_<sp>, n_<sp>                       computeSpeciesPrimitives of the state, num_species rows each
 *   viscosity, bulk_viscosity, thermal_cond_heavy, thermal_cond_elec      ComputeFluxTransportProperties
 *   diff_vel_<sp>                                nvel rows per species, species-major (grid functions on nvelfes); the rows
 *                                                past dim (the azimuthal one, axisymmetric) are zero, as the transport leaves them
 *   electric_cond                                SrcTrns of ComputeSourceTransportProperties
 *   momentum_tranfer_freq_<sp>                   SpeciesTrns (the spelling is the reference's); of one-temperature mixtures too
 *   rxn_rate_1 .. rxn_rate_R                     progress rates kf (prod n^nu' - prod n^nu'' / kC), NOT species sources
 * Point for point as the reference: the UNCLAMPED state, prim = Up and the gradients = gradUp of the state, Efield = 0, the
 * rates from the number densities ComputeSourceTransportProperties returns, Chemistry's temperature floor inside the rate
 * coefficients. */
typedef struct tpsrhs_vis_layout { /* AuxiliaryVisualizationIndexes: first ROW of each group, -1 = absent */
  int nrows;                        /* 4*nsp + nsp*nvel + 5 + num_reactions */
  int Xsp, Ysp, nsp_, FluxTrns, diffVel, SrcTrns, SpeciesTrns, rxn; /* rxn = -1 without reactions */
  int num_species, nvel, num_reactions;
} tpsrhs_vis_layout;
/* Host only, touches no device.  nvel = 3 when `axisymmetric` or dim == 3, else 2.  A NULL pointer, a dim other than
 * 2 / 3 or an axisymmetric dim 3: TPSRHS_ERR_INVALID_ARGUMENT; dry air (the reference skips the whole block for it) and the
 * table gas: TPSRHS_ERR_UNSUPPORTED. */
int tpsrhs_visualization_layout(const tpsrhs_physics *physics, int dim, int axisymmetric, tpsrhs_vis_layout *out);
/* visualization() of the reference (:4107-4112): refreshes the operator's Up and gradUp from x (tpsrhs_update_gradients,
 * halo exchange included on a partitioned mesh), then fills out.  x, out: DEVICE, out[nrows][NDofs] of
 * tpsrhs_visualization_layout for this operator; every row of every node is written.  Asynchronous on the operator's
 * stream, like tpsrhs_get_plasma_conductivity.  TPSRHS_ERR_UNSUPPORTED, never a fallback: dry air, the table gas, and an
 * operator with a mixing length set (the reference would route distance and radius through MixingLengthTransport). */
int tpsrhs_visualization_fields(tpsrhs_handle h, const double *x, double *out);

/* JouleHeating (src/forcing_terms.cpp:443-471): `joule_heating` is the DEVICE array of the
 * `joule_heating_` grid function (NDofs doubles, owned by the caller, read at every Mult; the EM solver
 * refreshes it between steps).  Positive entries are added to the total-energy equation and, for a
 * two-temperature mixture, to the electron-energy equation.  NULL disables the term. */
int tpsrhs_set_joule_heating(tpsrhs_handle h, const double *joule_heating);

/* ---- the flow side of the coupling to an electron Boltzmann solver (src/M2ulPhyS2Boltzmann.cpp) -------------------------
 * A reaction with reaction_models[r] = TPSRHS_GRIDFUNCTION_RXN (reactions/reactionN/model = bte) is the reference's
 * GridFunctionReaction (src/reaction.cpp:85-117, src/chemistry.cpp:89-91,133-139): its forward rate coefficient is read per
 * node from one component of a rate array.  The component -- bte/index, ReactionInput::indexInput -- is passed in
 * rate_params[0 + r * TPSRHS_MAXCHEMPARAMS]; a value that is not an integer >= 0: TPSRHS_ERR_INVALID_ARGUMENT at
 * tpsrhs_create.  Stoichiometry, reaction energy, detailed balance and the equilibrium constant are as for every reaction.
 *
 * M2ulPhyS::fetch (:89-101).  `rates` is a DEVICE array [num_components][size], byNODES, owned by the caller and read at every
 * Mult (like the array of tpsrhs_set_joule_heating; the kinetic solver refreshes it between steps).  Component c starts at
 * rates + c * size, as GridFunctionReaction::setGridFunction has it -- NOT as setData has it, which offsets by the size of
 * the PREVIOUS call (src/reaction.cpp:90-93).  NULL removes the array: an external reaction then has k_f = 0, as the
 * reference returns when data_ is null.  size != NDofs, num_components not greater than every configured component, or a
 * non-NULL array on an operator without such a reaction: TPSRHS_ERR_INVALID_ARGUMENT.  While an array is set the RK4 stages
 * take the unfused path, as with a forcing term.  A time-loop graph captured before the call is not replayed after it. */
int tpsrhs_set_reaction_rates(tpsrhs_handle h, const double *rates, int num_components, int64_t size);
/* M2ulPhyS::push (:40-87): what the Boltzmann solver gets.  x: DEVICE, the layout of tpsrhs_mult.  out: DEVICE
 * [num_species + 2][NDofs] -- rows 0 .. num_species-1 hold AVOGADRONUMBER * n_sp of computeNumberDensities of the UNCLAMPED
 * state (particles per m^3), then the heavy and the electron temperature of computeTemperaturesBase (the two rows are equal
 * for a one-temperature mixture).  1 <= num_species <= the mixture's species count, else TPSRHS_ERR_INVALID_ARGUMENT.
 * Asynchronous on the operator's stream.  Dry air and the table gas: TPSRHS_ERR_UNSUPPORTED. */
int tpsrhs_boltzmann_fields(tpsrhs_handle h, const double *x, int num_species, double *out);

/* ---- restart of a species plasma from an LTE solution (`io/restartFromLTE = True`) --------------------------------------
 * The reference reads only rho, rho u, rho E of such a restart file (the species rows and rhoE_e are optional,
 * src/M2ulPhyS.cpp:1842-1853), and M2ulPhyS::initilizeSpeciesFromLTE (:2388-2461) rebuilds every node with
 * PerfectMixture::GetSpeciesFromLTE -- a serial host loop that needs GSL and is compiled out of its CUDA and HIP builds.
 * Here both forms of that routine run on the device, for USER_DEFINED mixtures in the routine's species order: the ion of
 * charge +1 at num_species - 3, the electron at num_species - 2, the neutral background last, every species before the ion
 * an excited level of the neutral (src/equation_of_state.cpp:1952-1970).  Dry air, the table gas, and a mixture in another
 * order (a charged species below num_species - 3, no +1 ion at num_species - 3, no electron): TPSRHS_ERR_UNSUPPORTED, the
 * message names the species.  NULL handle or array, n < 0: TPSRHS_ERR_INVALID_ARGUMENT.  All refusals come before any
 * device work.  Both entry points are ordered on the operator's stream and synchronous on return.
 *
 * The tables: the thermo file's columns 3 (e) and 6 (R) over (T, rho) and the e_rev file's T over (e, rho)
 * (flow/lte/thermo_table, flow/lte/e_rev_table; src/M2ulPhyS.cpp:2414-2429).  Host pointers, copied for the duration of the
 * call.  The sound-speed table the reference also passes in is never read (src/equation_of_state.cpp:1944-2094) and is not
 * asked for.  Each table must satisfy tpsrhs_table2d and the energy must increase with T on every density line:
 * TPSRHS_ERR_INVALID_ARGUMENT otherwise; `energy` and `gas_constant` on different axes: TPSRHS_ERR_UNSUPPORTED (as
 * tpsrhs_lte2d). */
typedef struct tpsrhs_lte_restart {   /* flow/lte/thermo_table columns 3 and 6, flow/lte/e_rev_table */
  tpsrhs_table2d energy, gas_constant, temperature;
} tpsrhs_lte_restart;
/* num_not_converged: nodes whose Newton iteration for T did not converge in 20 steps (the reference prints a warning and goes
 * on with the last iterate, :2024-2027; so does this library).  num_invalid: nodes where the reference would have hit one of
 * its asserts -- T <= 0 in the Newton loop (:2014), n_e < 0, some n_sp < 0, |n_0 - sum n_sp| / n_0 >= 1e-14 (:2181-2186);
 * their rows hold what the arithmetic gave.  max_density_change = max |rho_new / rho - 1|: the tables and the mixture may
 * carry different excited levels, so T and p are kept and the density moves "a few tenths of a percent"; larger values point
 * to a mistake in the input (:2048-2057).  t_min, t_max: the extrema of the temperature found.  Reduced on the device in a
 * fixed order: the same state gives the same report. */
typedef struct tpsrhs_lte_restart_report {
  int64_t num_not_converged, num_invalid;
  double max_density_change, t_min, t_max;
} tpsrhs_lte_restart_report;
/* PerfectMixture::GetSpeciesFromLTE(T, p, n_sp), src/equation_of_state.cpp:2096-2187 (also the start of the reference's
 * low-Mach reacting solver, src/reactingFlow.cpp:1909-1921): the electron density from the Saha equation, the levels of the
 * neutral from the Boltzmann distribution with TPSRHS_SPECIES_DEGENERACY and TPSRHS_FORMATION_ENERGY, in the reference's
 * order of operations.  T [K], p [Pa]: DEVICE [n].  n_sp_out: DEVICE [num_species][n], mol/m^3. */
int tpsrhs_lte_composition(tpsrhs_handle h, int64_t n, const double *T, const double *p, double *n_sp_out);
/* PerfectMixture::GetSpeciesFromLTE(conserv, primit, tables) at every node (src/equation_of_state.cpp:1944-2094,
 * src/M2ulPhyS.cpp:2441-2455), then the species clamp of Check_Undershoot (:2526-2548) on the new state.  x: DEVICE
 * [num_equation][NDofs], the layout of tpsrhs_mult, updated in place: on entry only the rows 0 .. nvel + 1 (rho, rho u,
 * rho E of the LTE solution) are read, every row is written -- T from the tables by Newton, p = rho R(T, rho) T, the
 * composition at (T, p), then rho, rho u (velocity unchanged), rho E, rho Y_sp and, two temperatures, rhoE_e = n_e c_v,e T.
 * up_out: DEVICE [num_equation][NDofs] or NULL, the primitives of the new state (rho, u, T, n_sp, T_e = T).  report: HOST,
 * or NULL. */
int tpsrhs_species_from_lte(tpsrhs_handle h, const tpsrhs_lte_restart *tables, double *x, double *up_out,
                            tpsrhs_lte_restart_report *report);

/* ---- conservative positivity limiter (a replacement for Check_Undershoot the reference does not have) -------------------
 * After every step the reference sets negative species densities to zero (M2ulPhyS::Check_Undershoot,
 * src/M2ulPhyS.cpp:2522-2548); its own comment names the remedy it lacks ("the effect of oscillations can be mitigated by
 * employing a TVD scheme", :2522-2525).  That clamp adds mass with every firing.  This is the Zhang-Shu linear scaling
 * limiter, element by element: it leaves every element mean, and so every tpsrhs_integrate total, where it was.  Opt-in:
 * with no limiter configured nothing changes by a bit.  THE OPERATION, part of the contract:
 *   Weights.  W_n = int_K l_n dV on THE RULE of tpsrhs_integrate: NQ = p + 2 Gauss-Legendre points per direction, order-1
 *     geometry, the operator's Lagrange basis (Gauss-Legendre or Gauss-Lobatto nodes), |det J| at each point, times r_q
 *     when the operator is axisymmetric.  So sum_n W_n f_n equals tpsrhs_integrate(f).sum up to rounding for both basis /
 *     rule pairs; on the Gauss-Lobatto pair the W_n are NOT the nodal quadrature weights.  Computed once per operator on
 *     the device (the transpose of tpsrhs_integrate's interpolation, sum-factorised), kept in a [NDofs] buffer the
 *     operator owns, freed by tpsrhs_destroy.
 *   Row step.  Element K with N nodes, a row v and a floor f:  mean = sum W_n v_n / sum W_n;  m = min_n v_n, kept with
 *     `<`, so a NaN never wins.
 *       1. mean is NaN: the element is left as it is and not counted (the NaN census of the loop reports it).
 *       2. m >= f: untouched, nothing is written.
 *       3. else mean > f: theta = (mean - f) / (mean - m);  v_n <- mean + theta (v_n - mean);  then v_n <- fmax(v_n, f),
 *          which after the scaling can only move a value by rounding.  Counted in limited[row].
 *       4. else the mean itself is inadmissible and no conservative fix exists: v_n <- fmax(v_n, f), the reference's clamp
 *          for this element only.  Counted in clamped[row].
 *   Pressure step.  Dry air only, after the row steps, only when pressure_floor = f_p > 0.
 *     p(U) = (gamma - 1)(U[nvel+1] - 1/2 sum_{d=1..nvel} U[d]^2 / U[0]), gamma of tpsrhs_dry_air; Ubar the vector of the
 *     element means of all rows; pbar = p(Ubar), p_min = min_n p(U_n).  p_min >= f_p: nothing happens.  Else pbar > f_p:
 *     theta = (pbar - f_p) / (pbar - p_min), every row of the element is scaled as v_n <- vbar + theta (v_n - vbar);
 *     counted in pressure_limited.  p is concave in U for rho > 0, so p(U_n') >= (1 - theta) pbar + theta p(U_n) >= f_p up
 *     to rounding: no quadratic is solved.  Else the element is left untouched and counted in pressure_unfixable.
 * In the time loop (tpsrhs_limiter_configure): one step is the stage sequence followed by the limiter, in tpsrhs_step,
 * tpsrhs_rk4_step and every step of tpsrhs_advance / tpsrhs_advance_with (inside the captured step graph).  The limiter
 * replaces the clamp on the rows it lists: it must list all species rows or none (the clamp range stays contiguous).  The
 * statistics, probes, monitor and patch history see the limited state.  RK4 inside an advance runs unchained (x changes
 * after stage 4: every step starts with its own k_traces sweep).  dt of the next step comes from the last stage's
 * max_char_speed as without the limiter: the limiter does not feed it.  Element-local: partitioned meshes need nothing. */
typedef struct tpsrhs_limiter { /* replaces Check_Undershoot, src/M2ulPhyS.cpp:2522-2548 */
  int num_rows;                         /* -1: the rows Check_Undershoot clamps, [sp_first, sp_last) of the plan, floor 0 */
  int rows[TPSRHS_MAXEQUATIONS];
  double floors[TPSRHS_MAXEQUATIONS];
  double pressure_floor;                /* 0: off; > 0: dry air only, needs row 0 listed with a floor > 0 */
} tpsrhs_limiter;
typedef struct tpsrhs_limiter_report { /* what took Check_Undershoot's place, src/M2ulPhyS.cpp:2522-2548 */
  int64_t calls, limited[TPSRHS_MAXEQUATIONS], clamped[TPSRHS_MAXEQUATIONS], pressure_limited, pressure_unfixable;
} tpsrhs_limiter_report;                /* limited / clamped indexed by state row */
/* Refusals of the four entry points, all before any device work.  TPSRHS_ERR_INVALID_ARGUMENT: a NULL handle, x or out; a
 * row outside [0, neq) or listed twice; num_rows < -1 or > neq; a NaN floor; pressure_floor < 0 or NaN; pressure_floor > 0
 * without row 0 at a floor > 0; (configure only) some species rows listed but not all.  TPSRHS_ERR_UNSUPPORTED, with a
 * message: pressure_floor > 0 on a mixture or the table gas.  num_rows = -1 on an operator without species rows (dry air,
 * table gas) is a valid, empty limiter. */
/* The weights W_n (src/M2ulPhyS.cpp:2522-2548 has no counterpart).  w_out: DEVICE [NDofs]; synchronous on return. */
int tpsrhs_limiter_weights(tpsrhs_handle h, double *w_out /* DEVICE [NDofs] */);
/* One application of `lim` to x (DEVICE [num_equation][NDofs], in place; in place of src/M2ulPhyS.cpp:2522-2548),
 * asynchronous on the operator's stream.  Adds to the counters tpsrhs_limiter_read reports. */
int tpsrhs_limit(tpsrhs_handle h, const tpsrhs_limiter *lim, double *x /* DEVICE, in place */);
/* The limiter of the time loop (in place of the clamp of src/M2ulPhyS.cpp:2522-2548); NULL: off, the clamp is back.  A
 * step graph captured before the call is not replayed. */
int tpsrhs_limiter_configure(tpsrhs_handle h, const tpsrhs_limiter *lim /* NULL: off */);
/* The counters since the operator was created or since the last read with reset != 0 (elements per outcome, where
 * src/M2ulPhyS.cpp:2522-2548 counts nothing); calls: applications.  Integer sums: two runs give the same numbers.
 * Synchronises the stream. */
int tpsrhs_limiter_read(tpsrhs_handle h, tpsrhs_limiter_report *out, int reset);

/* ---- Legendre modal filter and smoothness sensor (the compressible solver of the reference has neither) ------------------
 * The exponential modal filter of Hesthaven & Warburton takes out the energy that piles up in the highest modes of an
 * under-resolved nodal DG solution before it becomes the undershoot the limiter above has to repair; the modal-decay sensor
 * of Persson & Peraire says, per element, where the solution is under-resolved.  Both are one small tensor contraction per
 * element, element-local (partitioned meshes need nothing), and do not look at the physics: every order 1 .. 5, both basis
 * / rule pairs, quads, hexes and axisymmetric operators, every gas model.  Opt-in: with no filter configured nothing
 * changes by a bit.  THE OPERATION, part of the contract, per element with N1 = p + 1 nodes per direction, xi_a in [0, 1]
 * the operator's own nodes (Gauss-Legendre or Gauss-Lobatto), lexicographic node order as everywhere:
 *   Modes.  V[a][k] = P_k(2 xi_a - 1), the Legendre polynomials, k = 0 .. p.  The modal coefficients of a nodal row u are
 *     u^ = (V^-1 x ... x V^-1) u, V^-1 along each of the dim directions.  V, V^-1 and F are formed on the host from the
 *     order and the basis, rounded to double, and go to the kernels by value.
 *   Filter.  sigma_k = 1 for k <= k_c = cutoff, sigma_k = exp(-alpha ((k - k_c) / (p - k_c))^s) for k > k_c, s = exponent.
 *     F = V diag(sigma) V^-1 and u~ = (F x ... x F) u.  With conservative != 0, afterwards
 *     u~_n += sum_n W_n (u_n - u~_n) / sum_n W_n with W_n the weights of tpsrhs_limiter_weights (the rule of
 *     tpsrhs_integrate, times r when the operator is axisymmetric): every element integral, and so every tpsrhs_integrate
 *     total, stays where it was on any mesh.  With conservative == 0 only the reference-space mean is kept (sigma_0 = 1),
 *     which is the physical mean on affine elements only.
 *   Shell energies and sensor of one scalar field.  gamma_k = 1 / (2k + 1);
 *     E_m = sum over the modes with max(i, j[, k]) = m of u^^2 gamma_i gamma_j [gamma_k], m = 0 .. p: the reference-space L2
 *     norm squared, split by the highest 1-D degree.  S = E_p / sum_m E_m; S = 0 when the sum is 0; S is NaN when the
 *     element holds a NaN.
 *   Selective filtering.  With sensor_row >= 0, S is computed from that row of the INCOMING state, before any row is
 *     written, and the element is filtered on all listed rows only if S > sensor_threshold (a NaN sensor: not filtered;
 *     sensor_threshold = +inf: never).  With sensor_row = -1 every element is filtered.  An element that is not filtered
 *     is not written.
 * In the time loop (tpsrhs_modal_filter_configure): one step is the stage sequence, then the filter, then the limiter when
 * one is configured, in tpsrhs_step, tpsrhs_rk4_step and every step of tpsrhs_advance / tpsrhs_advance_with (inside the
 * captured step graph).  The species clamp of the stage kernels runs BEFORE the filter, so a filter on species rows can
 * undershoot again: the limiter, which has the last word on the floors, is the remedy.  The statistics, probes, monitor
 * and patch history see the filtered (then limited) state.  RK4 inside an advance runs unchained, as with a limiter (x
 * changes after stage 4).  dt of the next step comes from the last stage's max_char_speed: the filter does not feed it. */
typedef struct tpsrhs_modal_filter {
  int num_rows;                       /* -1: every state row */
  int rows[TPSRHS_MAXEQUATIONS];
  int cutoff;                         /* k_c, 0 .. p-1 */
  double alpha;                       /* > 0, finite */
  int exponent;                       /* s >= 1 */
  int conservative;
  int sensor_row;                     /* -1: none */
  double sensor_threshold;
} tpsrhs_modal_filter;
typedef struct tpsrhs_modal_filter_report { int64_t calls, elements_seen, elements_filtered; } tpsrhs_modal_filter_report;
/* Refusals of the five entry points, all before any device work, TPSRHS_ERR_INVALID_ARGUMENT: a NULL handle, pointer or
 * struct; a row outside [0, neq) or listed twice; num_rows < -1 or > neq; cutoff outside 0 .. p-1; alpha <= 0, NaN or inf;
 * exponent < 1; sensor_row outside [-1, neq); a NaN threshold; nrows < 1; both outputs of tpsrhs_modal_energy NULL. */
/* out = (V^-1 x ... x V^-1) in (inverse == 0) or (V x ... x V) in (inverse != 0), row by row.  in, out: DEVICE
 * [nrows][NDofs]; in == out is allowed (otherwise they must not overlap).  Asynchronous on the operator's stream. */
int tpsrhs_modal_transform(tpsrhs_handle h, int inverse, int nrows, const double *in, double *out);
/* The shell energies and the sensor of one scalar field (DEVICE [NDofs]).  energy_out: DEVICE [ne][p+1] or NULL;
 * sensor_out: DEVICE [ne] or NULL; not both NULL.  Asynchronous on the operator's stream. */
int tpsrhs_modal_energy(tpsrhs_handle h, const double *field, double *energy_out, double *sensor_out);
/* One application of `f` to x (DEVICE [num_equation][NDofs], in place), one kernel launch, asynchronous on the operator's
 * stream.  Adds to the counters tpsrhs_modal_filter_read reports. */
int tpsrhs_modal_filter_apply(tpsrhs_handle h, const tpsrhs_modal_filter *f, double *x);
/* The filter of the time loop; NULL: off.  A step graph captured before the call is not replayed. */
int tpsrhs_modal_filter_configure(tpsrhs_handle h, const tpsrhs_modal_filter *f /* NULL: off */);
/* The counters since the operator was created or since the last read with reset != 0: applications, elements looked at,
 * elements filtered.  Integer sums: two runs give the same numbers.  Synchronises the stream. */
int tpsrhs_modal_filter_read(tpsrhs_handle h, tpsrhs_modal_filter_report *out, int reset);

/* Host-only view of the face topology tpsrhs_create derives from a mesh (the role of the
 * indirection arrays of src/M2ulPhyS.cpp:816-1486); touches no device.  Outputs (caller-allocated):
 *   face_nbr[ne*2*dim]   >= 0: trace slot (element*2*dim + local face) of the neighbour, slots
 *                        >= ne*2*dim are halo slots in shared-face order; < 0: -(bc index + 1)
 *   face_orient[ne*2*dim] 3-bit code (swap | flip_a<<1 | flip_b<<2) from my face frame to the
 *                        neighbour's (interior) or to the canonical frame (shared)
 *   shared_slot[nshared], shared_orient[nshared]: own slot / frame code of every shared face */
int tpsrhs_face_tables(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int32_t *face_nbr,
                       uint8_t *face_orient, int32_t *shared_slot, uint8_t *shared_orient);

const char *tpsrhs_status_string(int status);
const char *tpsrhs_last_error(void); /* thread-local text of the last failure */
const char *tpsrhs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TPSRHS_H_ */
