// augment_checks.hip -- the host side of csrc/augment.hip under AddressSanitizer + UBSan on the CPU (no GPU is used): every rejection
// of plipmi_warp_u8 happens before the handle is read or anything is launched, so a program without a device can walk all of them,
// the arithmetic at the edges of int and int64 included.  tests/test_augment_host.py builds it from augment.hip (sanitised) plus the
// library's other objects (as built) and runs it; it prints what failed and exits non-zero.
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
  alignas(8) static uint8_t px[64];
  alignas(8) static double co[16];
  alignas(8) static int32_t win[16];
  const int H = 37, W = 53;
  const int64_t pitch = 161, stride = 6001;
  const uint32_t fill = 127u | 5u << 8 | 250u << 16;
  REJECTS(plipmi_warp_u8(nullptr, px, 2, H, W, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "null handle");
  REJECTS(plipmi_warp_u8(h, px, -1, H, W, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "B -1");
  REJECTS(plipmi_warp_u8(h, px, INT_MIN, H, W, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "is negative");
  REJECTS(plipmi_warp_u8(h, px, 2, 0, W, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "a source of 0 x 53");
  REJECTS(plipmi_warp_u8(h, px, 2, H, -1, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "a source of 37 x -1");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, 0, 24, fill, px, nullptr), "an output of 0 x 24");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, 24, INT_MIN, fill, px, nullptr), "an output of 24 x");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, 158, stride, win, co, 0, 24, 24, fill, px, nullptr), "pitch_bytes 158");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, -161, stride, win, co, 0, 24, 24, fill, px, nullptr), "pitch_bytes -161");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, INT64_MIN, stride, win, co, 0, 24, 24, fill, px, nullptr), "pitch_bytes");
  REJECTS(plipmi_warp_u8(h, px, 2, INT_MAX, INT_MAX, 3ll * INT_MAX, stride, win, co, 0, 24, 24, fill, px, nullptr), "2 GiB");
  REJECTS(plipmi_warp_u8(h, px, 2, 65536, 10000, 32768, stride, win, co, 0, 24, 24, fill, px, nullptr), "2 GiB");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, INT64_MAX, stride, win, co, 0, 24, 24, fill, px, nullptr), "2 GiB");
  REJECTS(plipmi_warp_u8(h, px, 2, INT_MAX, 1, 1ll << 31, stride, win, co, 0, 24, 24, fill, px, nullptr), "2 GiB");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, -1, win, co, 0, 24, 24, fill, px, nullptr), "image_stride_bytes -1");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, INT64_MIN, win, co, 0, 24, 24, fill, px, nullptr), "image_stride_bytes");
  REJECTS(plipmi_warp_u8(h, px, 3, H, W, pitch, INT64_MAX / 2, win, co, 0, 24, 24, fill, px, nullptr), "bytes apart");
  REJECTS(plipmi_warp_u8(h, px, INT_MAX, H, W, pitch, INT64_MAX, win, co, 0, 24, 24, fill, px, nullptr), "bytes apart");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 2, 24, 24, fill, px, nullptr), "perspective 2");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, -1, 24, 24, fill, px, nullptr), "perspective -1");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, 24, 24, 1u << 24, px, nullptr), "fill_rgb 0x1000000");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, 24, 24, UINT32_MAX, px, nullptr), "fill_rgb");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, INT_MAX, INT_MAX, fill, px, nullptr), "an output image of");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 0, 32768, 21846, fill, px, nullptr), "an output image of 32768 x 21846");
  REJECTS(plipmi_warp_u8(h, nullptr, 2, H, W, pitch, stride, win, co, 0, 24, 24, fill, px, nullptr), "null src");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, nullptr, 0, 24, 24, fill, px, nullptr), "null coeffs");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, co, 1, 24, 24, fill, nullptr, nullptr), "null dst");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, win, reinterpret_cast<const double*>(px + 4), 0, 24, 24, fill, px, nullptr), "8-byte aligned");
  REJECTS(plipmi_warp_u8(h, px, 2, H, W, pitch, stride, reinterpret_cast<const int32_t*>(px + 2), co, 0, 24, 24, fill, px, nullptr), "4-byte aligned");
  // more workgroups than a grid holds: 2^20 outputs of 1024 x 1024 (PX = 4: 1024 workgroups each), and the byte kernel's four times as many
  REJECTS(plipmi_warp_u8(h, px, INT_MAX, H, W, pitch, 0, win, co, 0, 1024, 1024, fill, px, nullptr), "in one call");
  REJECTS(plipmi_warp_u8(h, px, 1 << 20, H, W, pitch, 0, win, co, 0, 1024, 1023, fill, px, nullptr), "in one call");
  // no outputs asked for: nothing to do, whatever the pointers are
  CHECK(plipmi_warp_u8(h, nullptr, 0, H, W, pitch, stride, nullptr, nullptr, 0, 24, 24, fill, nullptr, nullptr) == PLIPMI_OK);
  CHECK(plipmi_warp_u8(h, nullptr, 0, H, W, pitch, 0, nullptr, nullptr, 1, 1, 1, 0, nullptr, nullptr) == PLIPMI_OK);
  if (g_failed) {
    printf("%d augment check(s) FAILED\n", g_failed);
    return 1;
  }
  printf("augment checks passed\n");
  return 0;
}
