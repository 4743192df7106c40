// mg_look_quad.hip -- lookahead kernel forms of the compile-time robot scenes with 64 / blk lanes per env (5: robot
// only, 6: robot + one block; mg_lookahead.h)
#include "mg_lookahead.h"

MG_STEP_FORMS_QUAD(MG_LOOK_INSTANTIATE)
