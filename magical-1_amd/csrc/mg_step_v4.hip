// mg_step_v4.hip -- cooperative LDS step kernel, one env per 64-lane wavefront (form 4)
#include "mg_stepk.h"

MG_STEP_FORMS_COOP(MG_STEP_INSTANTIATE)

MG_PROF_READER(mg_prof_read_step_v4)
