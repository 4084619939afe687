// Post-processing passes of the plasma kernel family: dim 3, 3 velocity components, 8 species, ambipolar = false.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_3d_n8, 3, 3, 8, false)
