// mg_seq_v4.hip -- cooperative LDS step-sequence kernel, one env per 64-lane wavefront (form 4; mg_seq.h)
#include "mg_seq.h"

MG_STEP_FORMS_COOP(MG_SEQ_INSTANTIATE)
