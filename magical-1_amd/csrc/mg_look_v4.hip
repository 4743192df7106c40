// mg_look_v4.hip -- cooperative LDS lookahead kernel, one env per 64-lane wavefront (form 4; mg_lookahead.h)
#include "mg_lookahead.h"

MG_STEP_FORMS_COOP(MG_LOOK_INSTANTIATE)
