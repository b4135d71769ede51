// fe_fb.h — the opt-in forward-backward check of temporal tracks and stereo matches ("Forward-backward check"):
// track the result back with the same LK and ask whether it lands where it started.  ONE source for the decision: the kernel
// of fe_fb.hip (k_fb_points), the setter of the C ABI and the g++-compiled CPU harness (tests/cpp/fe_fb_test.cpp) all run
// these functions.  The backward track itself is l4_track (fe_lk.h), the function the forward track runs; what lives here is
// the comparison of its result with the origin: five float32 operations, each rounded to float32, compiled with
// -ffp-contract=off like everything else.
//   parameters  mode bits: 1 temporal, 2 stereo; thr2 = the threshold (level-0 pixels, 0 .. 64) squared in float32, t * t,
//               formed once on the host;
//   decision    dx = bx - ox, dy = by - oy; passes iff st != 0 and dx * dx + dy * dy <= thr2.  A NaN fails; an infinite
//               distance fails; threshold 0 passes only an exact return.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FFB_FN __host__ __device__ __forceinline__
#else
#define FFB_FN inline
#endif

#define FB_MAX_ERROR 64.0f
enum { FB_TEMPORAL = 1, FB_STEREO = 2 };      // mode bits

// What the forward-backward kernel reads of a stream beside its FeStreamDev: element i of a second array goes with descriptor
// i of the launch.  mode == 0 = this stream is not checked.
struct FeFbDev {
    float thr2_t, thr2_s;              // squared thresholds of the temporal / the stereo round trip
    int mode;
};

FFB_FN float fb_thr2(float t) { return t * t; }

// (bx, by): where the backward track ended, st its status; (ox, oy): the origin it should have returned to
FFB_FN bool fb_pass(float bx, float by, float ox, float oy, int st, float thr2) {
    const float dx = bx - ox, dy = by - oy;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    return st != 0 && d2 <= thr2;
}
