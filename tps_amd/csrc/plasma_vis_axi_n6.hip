// Post-processing passes of the plasma kernel family: dim 2, 3 velocity components, 6 species, ambipolar = false.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_axi_n6, 2, 3, 6, false)
