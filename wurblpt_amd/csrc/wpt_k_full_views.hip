/* wpt_k_full_views.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_VIEWS, false, false>: a batch of views of a scene at rest with any feature but measured BRDFs (the Sponza class) */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#define WPT_SINCOSF_POLY_BRANCH /* sincosf_ with the shared reduction but each polynomial behind its branch: both polynomials at once cost this kernel scratch (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_VIEWS, false, false, 4, false)
}
