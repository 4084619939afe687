// Post-processing passes of the plasma kernel family: dim 2, 2 velocity components, 4 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_2d_n4a, 2, 2, 4, true)
