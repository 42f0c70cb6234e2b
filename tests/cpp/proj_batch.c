/* Test helper: one fp32 projection function (the oracle's ho_project_exit_to_pixel, handed in as a pointer) over n directions, so that
 * tests/test_lens_model.py can ask it about millions of directions.  out5[5n] = {count, px0, py0, px1, py1}, absent hits 0. */
#include <stdint.h>

typedef struct {
  int32_t px, py, bump_landed;
} PixelHit;
typedef struct {
  PixelHit hits[2];
  int32_t count;
} ProjResult;
typedef ProjResult (*ProjectFn)(const void* params, float wx, float wy, float wz);

void proj_batch(ProjectFn fn, const void* params, const float* dirs, uint64_t n, int32_t* out5) {
  for (uint64_t i = 0; i < n; i++) {
    ProjResult r = fn(params, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    out5[5 * i] = r.count;
    for (int k = 0; k < 2; k++) {
      out5[5 * i + 1 + 2 * k] = k < r.count ? r.hits[k].px : 0;
      out5[5 * i + 2 + 2 * k] = k < r.count ? r.hits[k].py : 0;
    }
  }
}
