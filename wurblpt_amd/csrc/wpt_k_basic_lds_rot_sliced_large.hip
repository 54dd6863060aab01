/* wpt_k_basic_lds_rot_sliced_large.hip -- instantiates wpt_pathtrace_large<FEAT_BASIC | FEAT_ROTATED | FEAT_SLICED> (one variant per file: parallel builds) */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LARGE_LAUNCHER(FEAT_BASIC | FEAT_ROTATED | FEAT_SLICED, 4, LARGE_ORDERED)
}
