// Post-processing passes of the plasma kernel family: dim 3, 3 velocity components, 7 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_3d_n7a, 3, 3, 7, true)
