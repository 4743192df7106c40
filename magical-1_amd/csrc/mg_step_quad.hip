// mg_step_quad.hip -- step kernel forms of the compile-time robot scenes with 64 / blk lanes per env (5: robot
// only, 6: robot + one block; mg_stepq.h)
#include "mg_stepk.h"

MG_STEP_FORMS_QUAD(MG_STEP_INSTANTIATE)

MG_PROF_READER(mg_prof_read_step_quad)
