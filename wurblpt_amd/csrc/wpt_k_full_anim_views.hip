/* wpt_k_full_anim_views.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, false, false>: a batch of views with an exposure interval, animated
 * instances or an animated camera */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, false, false, 2, false)
}
