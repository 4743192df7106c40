// mg_look_hbm.hip -- HBM-state lookahead kernel (form 0; mg_lookahead.h)
#include "mg_lookahead.h"

MG_STEP_FORMS_HBM(MG_LOOK_INSTANTIATE)
