// Post-processing passes of the plasma kernel family: dim 3, 3 velocity components, 5 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_3d_n5a, 3, 3, 5, true)
