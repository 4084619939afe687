// Post-processing passes of the plasma kernel family: dim 2, 3 velocity components, 8 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_axi_n8a, 2, 3, 8, true)
