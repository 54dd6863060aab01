/* wpt_k_full_rgl_anim_tof.hip -- instantiates wpt_pathtrace<FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_TOF>: the time-of-flight
 * sensor for scenes with measured BRDFs, at rest or moving */
#define WPT_MATERIAL_CACHE /* wpt_blocks.h: the measured-BRDF model's incident-direction part is shared between scatter and the evaluation towards the light */
#define WPT_MATH_TABLES_IN_LDS /* this unit's kernels keep the tables of expf / powf in LDS (wpt_math.h) */
#include "wpt_pathtrace.inc.h"

namespace wptk {
WPT_PATHTRACE_LAUNCHER(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_TOF, false, false, 2, false)
}
