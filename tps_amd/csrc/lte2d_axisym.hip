// Kernel instantiations of the table gas with two-dimensional (T, rho) tables (WorkingFluid::LTE_FLUID, flow/lte/table_dim = 2),
// axisymmetric (dim 2, velocity components r, z, theta).
#include "launch.hpp"
#include "physics_dryair_axisym.hpp"

void pick_lte2d_axisym(tpsrhs_operator *op) { pick_order<2, Lte2dAxiPhys>(op); }
