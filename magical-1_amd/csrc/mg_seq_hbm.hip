// mg_seq_hbm.hip -- HBM-state step-sequence kernel (form 0; mg_seq.h)
#include "mg_seq.h"

MG_STEP_FORMS_HBM(MG_SEQ_INSTANTIATE)
