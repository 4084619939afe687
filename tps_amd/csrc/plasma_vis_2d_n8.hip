// Post-processing passes of the plasma kernel family: dim 2, 2 velocity components, 8 species, ambipolar = false.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_2d_n8, 2, 2, 8, false)
