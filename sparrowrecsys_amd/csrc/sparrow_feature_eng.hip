// sparrow_feature_eng.hip -- the pipelines that start from a ratings file or an embedding table, each as kernels (k_*.h) and a C ABI (api_*.h):
//   ratings -> training samples and the feature store's rows   k_feature_eng.h, api_feature_eng.h: sprk_feature_eng_workspace_bytes / sprk_feature_eng
//   ratings + item embeddings -> user embeddings               k_user_emb.h, api_user_emb.h: sprk_user_emb_workspace_bytes / sprk_user_emb
//   the movie catalogue                                        k_catalog.h, api_catalog.h: sprk_catalog_build_workspace_bytes / sprk_catalog_build / sprk_catalog_similar
//   ALS collaborative filtering                                k_als.h, api_als.h: sprk_als_workspace_bytes / sprk_als_fit / sprk_als_predict
//   item2vec: rating sequences and the skip-gram trainer       k_item2vec.h, api_item2vec.h: sprk_item_sequences / sprk_item_walks / sprk_skipgram_fit and their *_workspace_bytes
//   embedding LSH: buckets, a sorted index, approximate top-K  k_lsh.h, api_lsh.h: sprk_lsh_hash / sprk_lsh_build / sprk_lsh_query and sprk_lsh_build_workspace_bytes
//   samples -> a training and a test part, at random or by time  k_split.h, api_split.h: sprk_split_plan_workspace_bytes / sprk_split_plan / sprk_take_rows
//   top-K lists + held-out pairs -> ranking metrics            k_rank_eval.h, api_rank_eval.h: sprk_rank_eval_workspace_bytes / sprk_rank_eval
// and the unit that keeps the first one's store current:
//   new ratings -> the feature store's rows, in place          k_store_update.h, api_store_update.h: sprk_store_update_workspace_bytes / sprk_store_update
// The ratings pipelines count per id, scan, scatter into per-id segments and sort every segment, and the LSH index sorts one segment per
// hash table: k_segments.h has that device code and host_segments.h
// its launches, the workspace carver and the workspace check.  A translation unit of its own, like
// sparrow_metrics.hip: nothing here is used by the forward engine and nothing of the engine is used here.  Shares with the other units
// only host_common.h (the thread's error string behind sprk_last_error, HIP_TRY, the roctx ranges), which opens the kernels' namespace
// this file closes.
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
#include "k_segments.h"
#include "k_feature_eng.h"
#include "k_store_update.h"
#include "k_user_emb.h"
#include "k_catalog.h"
#include "k_als.h"
#include "k_item2vec.h"
#include "k_lsh.h"
#include "k_split.h"
#include "k_rank_eval.h"

}  // namespace sprk_dev
#pragma GCC visibility pop
using namespace sprk_dev;

#include "host_segments.h"
#include "api_feature_eng.h"
#include "api_store_update.h"
#include "api_user_emb.h"
#include "api_catalog.h"
#include "api_als.h"
#include "api_item2vec.h"
#include "api_lsh.h"
#include "api_split.h"
#include "api_rank_eval.h"
