// api_metrics.h -- C ABI: sprk_metrics_state_bytes / sprk_metrics_reset / sprk_metrics_update (model.evaluate's accumulators in device
// memory, k_metrics.h).  Part of sparrow_metrics.hip.  Every argument is checked before any
// device call; the calls launch on the caller's stream and return: no synchronisation, no memory of their own, and the device state
// is never read on the host.
extern "C" {

size_t sprk_metrics_state_bytes(int32_t num_thresholds) {
    if (num_thresholds < 2 || num_thresholds > SPRK_METRICS_MAX_THRESHOLDS) return 0;
    return 8 * mt_state_words(num_thresholds);
}

}  // extern "C"

namespace {
int metrics_check_state(const char* who, const void* state, size_t state_bytes, int32_t num_thresholds) {
    if (num_thresholds < 2 || num_thresholds > SPRK_METRICS_MAX_THRESHOLDS)
        return fail(SPRK_EINVAL, "%s: num_thresholds = %d outside [2, %d]", who, num_thresholds, SPRK_METRICS_MAX_THRESHOLDS);
    if (!state) return fail(SPRK_EINVAL, "%s: NULL state", who);
    if ((uintptr_t)state & 15) return fail(SPRK_EINVAL, "%s: state must start on a 16-byte boundary", who);
    if (state_bytes < sprk_metrics_state_bytes(num_thresholds))
        return fail(SPRK_EINVAL, "%s: state_bytes = %zu, %zu needed for %d thresholds", who, state_bytes, sprk_metrics_state_bytes(num_thresholds), num_thresholds);
    return SPRK_OK;
}
}  // namespace

extern "C" {

int sprk_metrics_reset(void* state, size_t state_bytes, int32_t num_thresholds, void* stream) {
    RoctxRange roctx_range_("sprk_metrics_reset");
    SPRK_TRY(metrics_check_state("metrics_reset", state, state_bytes, num_thresholds));
    hipLaunchKernelGGL(k_metrics_reset, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, (unsigned long long*)state, (int)num_thresholds);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

int sprk_metrics_update(void* state, size_t state_bytes, const float* scores, const void* labels, int32_t label_storage, int64_t label_stride,
                        int64_t n, void* stream) {
    RoctxRange roctx_range_("sprk_metrics_update");
    // every check before any device call.  T is the state's own word 0, which only the kernels read: the host checks the size against
    // the smallest state there is, the kernels against the T they find.
    SPRK_TRY(metrics_check_state("metrics_update", state, state_bytes, 2));
    int elem = 0;
    switch (label_storage) {
        case SPRK_COL_F32: case SPRK_COL_I32: elem = 4; break;
        case SPRK_COL_I64: elem = 8; break;
        case SPRK_COL_U8: case SPRK_COL_BOOL: elem = 1; break;
        default: return fail(SPRK_EINVAL, "metrics_update: label_storage = %d (float32, int32, int64, uint8 or bool labels)", label_storage);
    }
    if (label_stride <= 0 || label_stride % elem) return fail(SPRK_EINVAL, "metrics_update: label_stride = %lld is no positive multiple of the %d-byte label", (long long)label_stride, elem);
    if (n < 0) return fail(SPRK_EINVAL, "metrics_update: negative n");
    if (!scores) return fail(SPRK_EINVAL, "metrics_update: NULL scores");
    if (!labels) return fail(SPRK_EINVAL, "metrics_update: NULL labels");
    if ((uintptr_t)scores & 3) return fail(SPRK_EINVAL, "metrics_update: misaligned scores");
    if ((uintptr_t)labels & (uintptr_t)(elem - 1)) return fail(SPRK_EINVAL, "metrics_update: misaligned labels");
    if (n > 0 && label_stride > INT64_MAX / n) return fail(SPRK_EINVAL, "metrics_update: label_stride * n beyond 2^63 - 1");
    const unsigned long long words = state_bytes / 8;
    for (int64_t done = 0; done < n; done += MT_LAUNCH_MAX) {              // (one round unless n > 2^31)
        const long long m = n - done < MT_LAUNCH_MAX ? n - done : MT_LAUNCH_MAX;
        const float* s = scores + done;
        const unsigned char* l = (const unsigned char*)labels + done * label_stride;
        const long long slices = (m + MT_SLICE - 1) / MT_SLICE;
        const int G = (int)(slices < MT_MAX_GRID ? slices : MT_MAX_GRID);
        hipLaunchKernelGGL(k_metrics_update, dim3((unsigned)G), dim3(MT_THREADS), mt_lds_bytes(MT_MAX_T), (hipStream_t)stream, (unsigned long long*)state, words, s,
                           (int)(((uintptr_t)s & 15) == 0), l, (int)label_storage, (long long)label_stride, m);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_metrics_finish, dim3(1), dim3(MT_THREADS), (size_t)G * sizeof(double), (hipStream_t)stream, (unsigned long long*)state, words, G, m);
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}

}  // extern "C"
