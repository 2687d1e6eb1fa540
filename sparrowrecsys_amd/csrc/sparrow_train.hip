// sparrow_train.hip -- model.fit on the device: k_train.h (the kernels) and api_train.h (sprk_train_workspace_bytes / sprk_train_fit); k_train_fm.h and
// api_train_fm.h (sprk_train_fm_workspace_bytes / sprk_train_fm_fit) for DeepFM_v2, on the same schedule and the same sigmoid and Adam; k_train_din.h and
// api_train_din.h (sprk_train_din_workspace_bytes / sprk_train_din_fit) for DIN, whose schedule lets the columns of one table share a run; k_train_wide.h
// and api_train_wide.h (sprk_train_wide_workspace_bytes / sprk_train_wide_fit) for Wide&Deep: k_train.h's deep half plus the hashed cross's rows;
// k_train_pair.h and api_train_pair.h (sprk_train_pair_workspace_bytes / sprk_train_pair_fit) for the pair-dot DeepFM, on k_train.h's schedule;
// k_train_dien.h and api_train_dien.h (sprk_train_dien_workspace_bytes / sprk_train_dien_fit) for DIEN, on DIN's schedule and workspace;
// k_train_tower.h and api_train_tower.h (sprk_train_tower_workspace_bytes / sprk_train_tower_fit / sprk_tower_rows) for the two-tower NeuralCF, on
// k_train.h's schedule, and its towers' vectors.
// A translation unit of its own, like sparrow_metrics.hip and sparrow_feature_eng.hip: nothing here is used by the forward engine and
// nothing of the engine is used here.  The schedule is built with the segment code of the ratings pipelines (k_segments.h,
// host_segments.h); its kernels are not templates, so this unit's copies live in a namespace of their own and the linker sees two names.
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
namespace train_unit {
#include "k_segments.h"
#include "k_train.h"
#include "k_train_fm.h"
#include "k_train_din.h"
#include "k_train_dien.h"
#include "k_train_wide.h"
#include "k_train_pair.h"
#include "k_train_tower.h"
}  // namespace train_unit

}  // namespace sprk_dev
#pragma GCC visibility pop
using namespace sprk_dev;
using namespace sprk_dev::train_unit;

#include "host_segments.h"
#include "api_train.h"
#include "api_train_fm.h"
#include "api_train_din.h"
#include "api_train_dien.h"
#include "api_train_wide.h"
#include "api_train_pair.h"
#include "api_train_tower.h"
