/* wpt_k_full_transient.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_TRANSIENT, false, false>: the transient film for scenes
 * at rest that fetch the scene from HBM (the Sponza class); four waves per SIMD like its plain twin wpt_k_full.hip */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_TRANSIENT, false, false, 4, false)
}
