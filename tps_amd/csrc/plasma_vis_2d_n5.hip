// Post-processing passes of the plasma kernel family: dim 2, 2 velocity components, 5 species, ambipolar = false.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_2d_n5, 2, 2, 5, false)
