// sparrow_metrics.hip -- model.evaluate's accumulators in device memory: the kernels (k_metrics.h) and their C ABI (api_metrics.h:
// sprk_metrics_state_bytes / sprk_metrics_reset / sprk_metrics_update); and the exact ROC and PR areas over every distinct score
// (k_exact_auc.h, api_exact_auc.h: sprk_exact_auc_workspace_bytes / sprk_exact_auc_bin_bits / sprk_exact_auc), which bin, sort and scan
// with the segment code of the ratings pipelines (k_segments.h, host_segments.h) -- its kernels are not templates, so this unit's copies
// live in a namespace of their own, as sparrow_train.hip's do.  A translation unit of its own: nothing here is used by the
// forward engine and nothing of the engine is used here, so sparrow_hip.hip and the kernel-family units tu_1 .. tu_6.hip compile from
// the text they had before these calls existed.  Shares with them only host_common.h (the thread's error string behind sprk_last_error,
// HIP_TRY, the roctx ranges), which opens the kernels' namespace this file closes.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sparrow_hip.h"

#include "host_common.h"
#include "k_metrics.h"
namespace metrics_unit {
#include "k_segments.h"
#include "k_exact_auc.h"
}  // namespace metrics_unit

}  // namespace sprk_dev
#pragma GCC visibility pop
using namespace sprk_dev;
using namespace sprk_dev::metrics_unit;

#include "api_metrics.h"
#include "host_segments.h"
#include "api_exact_auc.h"
