// mg_seq_quad.hip -- step-sequence kernel forms of the compile-time robot scenes with 64 / blk lanes per env (5: robot
// only, 6: robot + one block; mg_seq.h)
#include "mg_seq.h"

MG_STEP_FORMS_QUAD(MG_SEQ_INSTANTIATE)
