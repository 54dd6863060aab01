/* wpt_k_full_anim_count_views.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, true, false>: a batch of views of a moving scene, with work counters */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, true, false, 2, false)
}
