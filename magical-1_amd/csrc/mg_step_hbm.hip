// mg_step_hbm.hip -- HBM-state step kernel (form 0)
#include "mg_stepk.h"

MG_STEP_FORMS_HBM(MG_STEP_INSTANTIATE)

MG_PROF_READER(mg_prof_read_step_hbm)
