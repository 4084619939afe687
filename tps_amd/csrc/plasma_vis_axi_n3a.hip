// Post-processing passes of the plasma kernel family: dim 2, 3 velocity components, 3 species, ambipolar = true.
#include "plasma_vis_family.hpp"
TPSRHS_PLASMA_VIS_FAMILY(pick_plasma_vis_axi_n3a, 2, 3, 3, true)
