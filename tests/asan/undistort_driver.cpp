// Host-side sanitizer driver for the lens-undistortion entries of include/adfp.h (tests/test_undistort_sanitizer_host.py builds the
// library with its host translation instrumented, as tests/asan/build_and_run.sh does, and runs this program).  adfp_undistort_map
// is host code that converts doubles to int: the maps below hold positions far beyond int32 and non-finite ones, which the
// contract clamps or replaces before the conversion.  The device entries are walked through their argument errors only.
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

#include "adfp.h"

static int failed = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failed; } \
    } while (0)

int main() {
    const int h = 37, w = 53;
    std::vector<int> map(2 * h * w + 2, -7);                       // two guard entries behind the map
    const double tum[5] = {0.2624, -0.9531, -0.0054, 0.0026, 1.1633};
    EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, tum, 5, map.data()) == 0);
    EXPECT(map[2 * h * w] == -7 && map[2 * h * w + 1] == -7);
    // zero coefficients: the identity in 1/32 pixels
    const double zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int n : {4, 5, 8}) {
        EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, zero, n, map.data()) == 0);
        bool same = true;
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) same = same && map[2 * (v * w + u)] == 32 * u && map[2 * (v * w + u) + 1] == 32 * v;
        EXPECT(same);
    }
    // positions of 1e12 pixels and more: clamped to +-2^30 before the conversion
    const double huge[4] = {1e14, 0, 0, 0};
    EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, huge, 4, map.data()) == 0);
    int lo = 0, hi = 0;
    for (int i = 0; i < 2 * h * w; ++i) { lo += map[i] == -(1 << 30); hi += map[i] == (1 << 30); }
    EXPECT(lo > 100 && hi > 100);
    // overflow to infinity and a zero denominator: the sentinel, in both entries
    const double inf_k[4] = {1e308, 1e308, 0, 0};
    EXPECT(adfp_undistort_map(h, w, 1e-3, 1e-3, 25.5, 17.5, inf_k, 4, map.data()) == 0);
    int sentinels = 0;
    for (int i = 0; i < h * w; ++i) {
        EXPECT((map[2 * i] == INT_MIN) == (map[2 * i + 1] == INT_MIN));
        sentinels += map[2 * i] == INT_MIN;
    }
    EXPECT(sentinels > h * w / 2);
    const double pole[8] = {0, 0, 0, 0, 0, -4.0, 0, 0};
    EXPECT(adfp_undistort_map(2, 3, 2.0, 2.0, 1.0, 0.0, pole, 8, map.data()) == 0);
    EXPECT(map[0] == INT_MIN && map[1] == INT_MIN && map[2] == 32 && map[3] == 0);
    EXPECT(map[2 * h * w] == -7 && map[2 * h * w + 1] == -7);
    // argument errors
    for (int n : {-1, 0, 3, 6, 7, 9, 12, 14}) EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, zero, n, map.data()) == ADFP_E_UNSUPPORTED);
    EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, nullptr, 5, map.data()) == ADFP_E_ARG);
    EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, 25.5, 17.5, zero, 5, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_map(0, w, 40.0, 41.0, 25.5, 17.5, zero, 5, map.data()) == ADFP_E_ARG);
    EXPECT(adfp_undistort_map(h, 32769, 40.0, 41.0, 25.5, 17.5, zero, 5, map.data()) == ADFP_E_UNSUPPORTED);
    EXPECT(adfp_undistort_map(h, w, 0.0, 41.0, 25.5, 17.5, zero, 5, map.data()) == ADFP_E_ARG);
    EXPECT(adfp_undistort_map(h, w, 40.0, NAN, 25.5, 17.5, zero, 5, map.data()) == ADFP_E_ARG);
    EXPECT(adfp_undistort_map(h, w, 40.0, 41.0, INFINITY, 17.5, zero, 5, map.data()) == ADFP_E_ARG);
    // the device entries refuse on the host before any launch (the pointers are opaque and never dereferenced)
    adfp_ingest_geom g = {h, w, h, w, 0, 0, 0, 1, 0, 0, 6553.5f, 1.0f};
    void* p = (void*)(size_t)64;
    adfp_ingest_job job = {(const unsigned char*)p, p, p, (float*)p};
    EXPECT(adfp_ingest_frames_undistort(nullptr, (const int*)p, 1, &job, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_ingest_frames_undistort(&g, (const int*)p, -1, &job, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_ingest_frames_undistort(&g, (const int*)p, 1, nullptr, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_ingest_frames_undistort(&g, (const int*)(size_t)68, 1, &job, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_ingest_frames_undistort(&g, (const int*)p, ADFP_INGEST_MAX_JOBS + 1, &job, nullptr) == ADFP_E_UNSUPPORTED);
    EXPECT(adfp_ingest_frames_undistort(&g, (const int*)p, 0, nullptr, nullptr) == 0);
    EXPECT(adfp_undistort_image(nullptr, (const int*)p, h, w, (unsigned char*)p, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_image((const unsigned char*)p, nullptr, h, w, (unsigned char*)p, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_image((const unsigned char*)p, (const int*)p, h, w, nullptr, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_image((const unsigned char*)p, (const int*)(size_t)68, h, w, (unsigned char*)p, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_image((const unsigned char*)p, (const int*)p, 0, w, (unsigned char*)p, nullptr) == ADFP_E_ARG);
    EXPECT(adfp_undistort_image((const unsigned char*)p, (const int*)p, h, 32769, (unsigned char*)p, nullptr) == ADFP_E_UNSUPPORTED);
    std::printf("undistort sanitizer driver: %d failed expectations\n", failed);
    return failed ? 1 : 0;
}
