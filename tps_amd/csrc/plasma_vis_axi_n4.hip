// Post-processing passes of the plasma kernel family: dim 2, 3 velocity components, 4 species, ambipolar = false.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_axi_n4, 2, 3, 4, false)
