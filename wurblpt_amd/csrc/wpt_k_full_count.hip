/* wpt_k_full_count.hip -- instantiates wpt_pathtrace<FEAT_ALL, true, false> (one variant per file: parallel builds) */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#define WPT_SINCOSF_SEPARATE /* sincosf_ as sinf_ + cosf_: either fused form costs this kernel scratch (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL, true, false, 2, false)
}
