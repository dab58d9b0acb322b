// region_checks.hip -- the host side of csrc/region.hip under AddressSanitizer + UBSan on the CPU (no GPU is used): every rejection
// of plipmi_region_select / plipmi_region_gather happens before the handle is read or anything is launched, so a program without a
// device can walk all of them, the arithmetic at the edges of int included.  tests/test_region_host.py builds it from region.hip
// (sanitised) plus the library's other objects (as built) and runs it; it prints what failed and exits non-zero.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "../../include/plipmi.h"

static int g_failed = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d  %s   [last error: %s]\n", __FILE__, __LINE__, #cond, plipmi_last_error()); } \
  } while (0)
static bool err_has(const char* s) { return strstr(plipmi_last_error(), s) != nullptr; }
#define REJECTS(call, text) do { CHECK((call) == PLIPMI_ERR_INVALID); CHECK(err_has(text)); } while (0)

int main() {
  plipmi_handle h = reinterpret_cast<plipmi_handle>(1);      // never read: every call below returns from its checks
  static uint8_t px[16];
  static int32_t i32[16];
  const int H = 200, W = 331;
  const int64_t pitch = 993;
  // ---- plipmi_region_select
  REJECTS(plipmi_region_select(nullptr, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "null handle");
  REJECTS(plipmi_region_select(h, nullptr, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "null region");
  REJECTS(plipmi_region_select(h, px, 0, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "a region of 0 x 331");
  REJECTS(plipmi_region_select(h, px, H, -1, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "a region of 200 x -1");
  REJECTS(plipmi_region_select(h, px, H, W, 992, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "pitch_bytes 992");
  REJECTS(plipmi_region_select(h, px, H, W, -993, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "pitch_bytes -993");
  REJECTS(plipmi_region_select(h, px, INT_MAX, INT_MAX, 3ll * INT_MAX, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "4 GiB");
  REJECTS(plipmi_region_select(h, px, 65536, 21845, 65536, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "4 GiB");
  REJECTS(plipmi_region_select(h, px, H, W, INT64_MAX, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "4 GiB");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 0, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "tile 0");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 0, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "stride 0");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, -1, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "origin (-1, 0)");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, -1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "a grid of -1 x 1");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, INT_MAX, INT_MAX, 18, 25, 235, 1, i32, i32, i32, nullptr), "a grid of");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 4, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "end at (256, 64)");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 6, 18, 25, 235, 1, i32, i32, i32, nullptr), "end at (64, 384)");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 137, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "end at (201, 64)");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, INT_MAX, 2, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "outside the 200 x 331 region");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, INT_MAX, INT_MAX, INT_MAX, 1, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "outside the 200 x 331 region");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 256, 25, 235, 1, i32, i32, i32, nullptr), "sat_min 256");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, -1, 235, 1, i32, i32, i32, nullptr), "luma_min -1");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 256, 1, i32, i32, i32, nullptr), "luma_max 256");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, -1, i32, i32, i32, nullptr), "min_count -1");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, i32, nullptr, nullptr), "null n_kept");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, nullptr, i32, i32, nullptr), "null counts/kept");
  REJECTS(plipmi_region_select(h, px, H, W, pitch, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, i32, nullptr, i32, nullptr), "null counts/kept");
  REJECTS(plipmi_region_select(h, px, 32769, 32769, 98307, 0, 0, 32769, 1, 1, 1, 18, 25, 235, 1, i32, i32, i32, nullptr), "tile 32769");
  // ---- plipmi_region_gather
  REJECTS(plipmi_region_gather(nullptr, px, H, W, pitch, 0, 0, 64, 64, 1, i32, 0, 1, px, nullptr), "null handle");
  REJECTS(plipmi_region_gather(h, nullptr, H, W, pitch, 0, 0, 64, 64, 1, i32, 0, 1, px, nullptr), "null region");
  REJECTS(plipmi_region_gather(h, px, H, W, 992, 0, 0, 64, 64, 1, i32, 0, 1, px, nullptr), "pitch_bytes 992");
  REJECTS(plipmi_region_gather(h, px, 65536, 21845, 65536, 0, 0, 64, 64, 1, i32, 0, 1, px, nullptr), "4 GiB");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 0, 64, 1, i32, 0, 1, px, nullptr), "tile 0");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 0, 1, i32, 0, 1, px, nullptr), "stride 0");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, -5, 64, 64, 1, i32, 0, 1, px, nullptr), "origin (0, -5)");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, -1, i32, 0, 1, px, nullptr), "a grid of 3 x -1");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 6, i32, 0, 1, px, nullptr), "end at (192, 384)");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 201, 201, 1, i32, 0, 1, px, nullptr), "empty grid");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 0, i32, 0, 1, px, nullptr), "empty grid");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, INT_MAX, 0, 64, 64, 1, i32, 0, 1, px, nullptr), "empty grid");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, i32, -1, 1, px, nullptr), "first -1");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, i32, 0, -1, px, nullptr), "B -1");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, i32, 10, 6, px, nullptr), "kept[10 .. 16)");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, i32, INT_MAX, INT_MAX, px, nullptr), "of a grid of 15 tiles");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, nullptr, 0, 1, px, nullptr), "null kept/dst");
  REJECTS(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, i32, 0, 1, nullptr, nullptr), "null kept/dst");
  REJECTS(plipmi_region_gather(h, px, 16385, 16385, 49155, 0, 0, 16385, 16385, 1, i32, 0, 1, px, nullptr), "tile 16385");
  // no tiles asked for: nothing to do, whatever the list and the destination are
  CHECK(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 64, 64, 5, nullptr, 0, 0, nullptr, nullptr) == PLIPMI_OK);
  CHECK(plipmi_region_gather(h, px, H, W, pitch, 0, 0, 201, 201, 0, nullptr, 0, 0, nullptr, nullptr) == PLIPMI_OK);
  if (g_failed) {
    printf("%d region check(s) FAILED\n", g_failed);
    return 1;
  }
  printf("region checks passed\n");
  return 0;
}
