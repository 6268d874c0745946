// The frame-ingestion part of libadfp as a translation unit of its own (csrc/adfp_ingest.h with the launch check of
// csrc/adfp_kernels.hip), for tests/test_undistort_sanitizer_host.py: seconds to build with the host side instrumented.
#include <hip/hip_runtime.h>

#define ADFP_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

#include "adfp_ingest.h"
