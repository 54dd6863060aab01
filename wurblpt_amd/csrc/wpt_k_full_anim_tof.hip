/* wpt_k_full_anim_tof.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_ANIM | FEAT_TOF, false, false>: the time-of-flight
 * sensor for scenes without measured BRDFs with an exposure interval or animated instances */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_ANIM | FEAT_TOF, false, false, 2, false)
}
