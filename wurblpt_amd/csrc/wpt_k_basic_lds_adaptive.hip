/* wpt_k_basic_lds_adaptive.hip -- instantiates wpt_pathtrace<FEAT_BASIC | FEAT_ADAPTIVE, false, true>: adaptive sampling of a scene of the basic feature set small enough for LDS (the Cornell class) */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_BASIC | FEAT_ADAPTIVE, false, true, 4, false)
}
