/* wpt_k_basic_lds_tof.hip -- instantiates wpt_pathtrace<FEAT_BASIC | FEAT_TWOSIDED | FEAT_SPOT | FEAT_TOF, false, true>: the
 * time-of-flight sensor for scenes of the basic feature set, ToF lights and two-sided materials small enough for LDS; four
 * workgroups per CU like its siblings, without the rotated copies of the corners */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_BASIC | FEAT_TWOSIDED | FEAT_SPOT | FEAT_TOF, false, true, 4, false)
}
