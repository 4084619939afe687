// Post-processing passes of the plasma kernel family: dim 3, 3 velocity components, 8 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_3d_n8a, 3, 3, 8, true)
