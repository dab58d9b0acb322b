// host_checks.hip -- the HIP-free half of libplipmi's host code, run under AddressSanitizer + UBSan on the CPU (no GPU is used):
// plipmi_create's validation, the early returns of every export, the hook setters, the pass arithmetic and -- through
// csrc/handle_host.h directly -- shape resolution and the two-pass slab carving.  tests/test_native_host.py builds it from the host
// translation units (sanitised) plus the library's kernel objects (as built) and runs it; it prints what failed and exits non-zero.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "handle_host.h"
#include "resize_ragged.h"

using namespace plipmi;

static int g_failed = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d  %s   [last error: %s]\n", __FILE__, __LINE__, #cond, plipmi_last_error()); } \
  } while (0)
static bool err_has(const char* s) { return strstr(plipmi_last_error(), s) != nullptr; }
#define REJECTS(call, text) do { CHECK((call) == PLIPMI_ERR_INVALID); CHECK(err_has(text)); } while (0)

struct Arch { const char* name; int image, patch, vw, vl, vh, vmlp, vocab, ctx, tw, tl, th, tmlp, proj, max_batch; };
static const Arch kTiny = {"tiny", 64, 16, 128, 2, 2, 256, 512, 16, 128, 2, 2, 256, 64, 8};
static const Arch kVitB32 = {"ViT-B/32", 224, 32, 768, 12, 12, 3072, 49408, 77, 512, 12, 8, 2048, 512, 256};
static const Arch kVitL14_336 = {"ViT-L/14@336px", 336, 14, 1024, 24, 16, 4096, 49408, 77, 768, 12, 12, 3072, 768, 64};
struct Variant { const char* name; int dtype, flags; };
static const Variant kVariants[] = {{"f32", PLIPMI_F32, 0}, {"bf16 folded", PLIPMI_BF16, 0},
                                    {"bf16 dense last block", PLIPMI_BF16, PLIPMI_FLAG_DENSE_LAST_BLOCK},
                                    {"bf16 separate LayerNorm", PLIPMI_BF16, PLIPMI_FLAG_SEPARATE_LAYERNORM}};
// slab sizes of the tiny config at max_batch 8 as computed by the commit before the handle was split into model + workspace
// (one slab [weights | workspace] per created handle, the workspace alone per clone), in kVariants order
static const size_t kTinyCreateSlab[] = {4808704, 2959104, 2934016, 2893824};
static const size_t kTinyCloneSlab[] = {1882112, 1277696, 1252608, 1212416};

static plipmi_config config_of(const Arch& a, const Variant& v) {
  plipmi_config g;
  memset(&g, 0, sizeof(g));
  g.struct_size = sizeof(g);
  g.image_size = a.image; g.patch_size = a.patch; g.v_width = a.vw; g.v_layers = a.vl; g.v_heads = a.vh; g.v_mlp = a.vmlp;
  g.vocab_size = a.vocab; g.context_length = a.ctx; g.t_width = a.tw; g.t_layers = a.tl; g.t_heads = a.th; g.t_mlp = a.tmlp;
  g.projection_dim = a.proj; g.layer_norm_eps = 1e-5f; g.compute_dtype = v.dtype; g.max_batch = a.max_batch; g.flags = v.flags;
  return g;
}

// ---- plipmi_create: every rejection in front of the device query ------------------------------------------------------------
static void check_create_validation() {
  plipmi_weights w;
  memset(&w, 0, sizeof(w));
  plipmi_handle h = reinterpret_cast<plipmi_handle>(1);
  const plipmi_config base = config_of(kTiny, kVariants[1]);
  auto rejects = [&](const std::function<void(plipmi_config&)>& edit, const char* text) {
    plipmi_config g = base;
    edit(g);
    h = reinterpret_cast<plipmi_handle>(1);
    const int rc = plipmi_create(&g, &w, nullptr, &h);
    if (rc != PLIPMI_ERR_INVALID || !err_has(text) || h != nullptr) {
      ++g_failed;
      printf("FAILED plipmi_create: expected a rejection naming \"%s\", got rc %d \"%s\"\n", text, rc, plipmi_last_error());
    }
  };
  REJECTS(plipmi_create(nullptr, &w, nullptr, &h), "null argument");
  REJECTS(plipmi_create(&base, nullptr, nullptr, &h), "null argument");
  REJECTS(plipmi_create(&base, &w, nullptr, nullptr), "null argument");
  // struct_size: below the members every version has had, just past the library's own
  const int min_size = (int)(offsetof(plipmi_config, max_batch) + sizeof(int32_t));
  rejects([&](plipmi_config& g) { g.struct_size = min_size - 4; }, "struct_size");
  rejects([&](plipmi_config& g) { g.struct_size = 0; }, "struct_size");
  rejects([&](plipmi_config& g) { g.struct_size = -8; }, "struct_size");
  rejects([&](plipmi_config& g) { g.struct_size = (int)sizeof(plipmi_config) + 4; }, "struct_size");
  {  // at both ends of the range the struct is read at the caller's size: members past it are defaults, not garbage
    plipmi_config g, out;
    memset(&g, 0xff, sizeof(g));
    const plipmi_config good = base;
    memcpy(&g, &good, (size_t)min_size);
    g.struct_size = min_size;
    CHECK(validate_config(&g, &out) == PLIPMI_OK);
    CHECK(out.struct_size == (int)sizeof(plipmi_config) && out.max_batch == base.max_batch);
    CHECK(out.flags == 0 && out.graph_batch == 0 && out.text_f16_layers == 0 && out.pass_batch == 0);
    g = base;
    CHECK(validate_config(&g, &out) == PLIPMI_OK && memcmp(&g, &out, sizeof(g)) == 0);
  }
  rejects([](plipmi_config& g) { g.compute_dtype = 3; }, "compute_dtype");
  rejects([](plipmi_config& g) { g.compute_dtype = -1; }, "compute_dtype");
  rejects([](plipmi_config& g) { g.flags = 1 << 20; }, "unknown bits");
  rejects([](plipmi_config& g) { g.flags = PLIPMI_FLAG_TEXT_TOWER_F16; g.compute_dtype = PLIPMI_F16; }, "PLIPMI_FLAG_TEXT_TOWER_F16");
  rejects([](plipmi_config& g) { g.flags = PLIPMI_FLAG_TEXT_TOWER_F16; g.compute_dtype = PLIPMI_F32; }, "PLIPMI_FLAG_TEXT_TOWER_F16");
  rejects([](plipmi_config& g) { g.text_f16_layers = -1; }, "text_f16_layers");
  rejects([](plipmi_config& g) { g.text_f16_layers = g.t_layers + 1; }, "text_f16_layers");
  rejects([](plipmi_config& g) { g.text_f16_layers = 1; g.compute_dtype = PLIPMI_F16; }, "text_f16_layers");
  rejects([](plipmi_config& g) { g.v_heads = 0; }, "head_dim");
  rejects([](plipmi_config& g) { g.t_heads = -2; }, "head_dim");
  rejects([](plipmi_config& g) { g.v_heads = 4; }, "head_dim");
  rejects([](plipmi_config& g) { g.t_width = 256; }, "head_dim");
  rejects([](plipmi_config& g) { g.patch_size = 0; }, "patch_size");
  rejects([](plipmi_config& g) { g.patch_size = 24; }, "patch_size");
  rejects([](plipmi_config& g) { g.v_width = 192; g.v_heads = 3; }, "multiples of 128");
  rejects([](plipmi_config& g) { g.t_width = 64; g.t_heads = 1; }, "multiples of 128");
  rejects([](plipmi_config& g) { g.v_mlp = 200; }, "multiples of 128");
  rejects([](plipmi_config& g) { g.t_mlp = 64; }, "multiples of 128");
  rejects([](plipmi_config& g) { g.v_width = 2176; g.v_heads = 34; }, "width > 2048");
  rejects([](plipmi_config& g) { g.t_width = 2176; g.t_heads = 34; }, "width > 2048");
  rejects([](plipmi_config& g) { g.projection_dim = 1025; }, "projection_dim");
  rejects([](plipmi_config& g) { g.projection_dim = 0; }, "projection_dim");
  rejects([](plipmi_config& g) { g.max_batch = 0; }, "non-positive");
  rejects([](plipmi_config& g) { g.v_layers = 0; }, "non-positive");
  rejects([](plipmi_config& g) { g.t_layers = 0; g.text_f16_layers = 0; }, "non-positive");
  rejects([](plipmi_config& g) { g.context_length = 0; }, "non-positive");
  rejects([](plipmi_config& g) { g.vocab_size = -5; }, "non-positive");
  rejects([](plipmi_config& g) { g.image_size = 528; g.patch_size = 16; }, "1024 tokens");   // 33 x 33 + 1
  rejects([](plipmi_config& g) { g.context_length = 1025; }, "1024 tokens");
  {  // a config that passes all of it reaches the device query -- and, where there is no device, stops there
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
      h = reinterpret_cast<plipmi_handle>(1);
      CHECK(plipmi_create(&base, &w, nullptr, &h) == PLIPMI_ERR_NODEVICE);
      CHECK(err_has("no HIP device visible") && h == nullptr);
    } else {
      printf("note: a HIP device is visible; the PLIPMI_ERR_NODEVICE return of plipmi_create is not exercised\n");
    }
  }
}

// a handle object as the constructor paths shape it, without a workspace: enough for everything that returns before a HIP call
static std::unique_ptr<plipmi_engine> shaped_handle(const Arch& a, const Variant& v, std::shared_ptr<Model>* model_out = nullptr) {
  plipmi_config g;
  const plipmi_config in = config_of(a, v);
  if (validate_config(&in, &g) != PLIPMI_OK) { ++g_failed; printf("FAILED: %s / %s does not validate: %s\n", a.name, v.name, plipmi_last_error()); }
  auto m = std::make_shared<Model>();
  init_model(m.get(), g);
  if (model_out) *model_out = m;
  auto e = std::make_unique<plipmi_engine>(m);
  shape_handle(e.get(), g.max_batch, g.image_size, g.image_size);
  return e;
}

// ---- exports: what they return before their first HIP call ----------------------------------------------------------------------
static void check_early_returns() {
  plipmi_handle out = reinterpret_cast<plipmi_handle>(1);
  float f[8] = {0};
  int32_t i32[8] = {0};
  int64_t i64[8] = {0};
  uint8_t u8[8] = {0};
  double d[8] = {0};
  alignas(16) float x16[8] = {0};
  int n = 0;
  plipmi_kernel_stat rows[2];
  plipmi_probe_info info;
  CHECK(plipmi_version() == PLIPMI_VERSION);
  // null handles
  CHECK(strcmp(plipmi_device_name(nullptr), "") == 0);
  plipmi_destroy(nullptr);
  REJECTS(plipmi_clone(nullptr, &out), "null argument");
  REJECTS(plipmi_clone_resolution(nullptr, 64, 64, 0, &out), "null argument");
  REJECTS(plipmi_encode_image(nullptr, f, 1, f, 0, nullptr), "null handle");
  REJECTS(plipmi_encode_image_u8(nullptr, u8, 1, f, 0, nullptr), "null handle");
  REJECTS(plipmi_encode_text(nullptr, i64, nullptr, 1, 2, f, 0, nullptr), "null handle");
  REJECTS(plipmi_check_async(nullptr), "null handle");
  REJECTS(plipmi_set_graph_batch(nullptr, 4), "null handle");
  CHECK(plipmi_get_pass_batch(nullptr) == 0);
  REJECTS(plipmi_streams_overlap(nullptr, nullptr, nullptr, f), "bad argument");
  REJECTS(plipmi_set_latency_batch(nullptr, 8), "null handle");
  REJECTS(plipmi_set_text_packing(nullptr, 1), "null handle");
  REJECTS(plipmi_tower_shape(nullptr, 0, i32), "null handle/shape");
  REJECTS(plipmi_encode_tower_outputs(nullptr, 0, f, nullptr, 1, 2, f, nullptr, nullptr, nullptr, nullptr), "null handle");
  REJECTS(plipmi_debug_hidden(nullptr, 0, 0, f, 1, f, nullptr), "null handle");
  REJECTS(plipmi_l2_normalize(nullptr, f, 1, 4, nullptr), "bad argument");
  REJECTS(plipmi_logits(nullptr, f, 1, f, 1, 4, 1.f, f, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_topk(nullptr, f, 1, 4, 1, i64, nullptr), "bad argument");
  REJECTS(plipmi_resize_crop_u8(nullptr, u8, 1, 4, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0, 4, u8, u8, nullptr), "bad argument");
  REJECTS(plipmi_resize_crop_u8_ragged(nullptr, u8, 8, i64, i32, i64, i32, 1, 2, 0, 4, u8, 8, u8, nullptr), "bad argument");
  REJECTS(plipmi_similarity_topk(nullptr, f, 1, f, 1, 32, 1, i64, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_probe_fit(nullptr, x16, 4, 4, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "null handle");
  REJECTS(plipmi_probe_predict(nullptr, x16, 4, 4, f, 1, nullptr, i32, nullptr), "null handle");
  REJECTS(plipmi_probe_loss_grad(nullptr, x16, 4, 4, i32, 1, f, f, 1.f, f, d, f, nullptr), "null handle");
  REJECTS(plipmi_profile_enable(nullptr, 1), "null handle");
  REJECTS(plipmi_profile_read(nullptr, rows, 2, &n), "bad argument");

  // a shaped handle: the argument checks behind the null-handle test
  auto eh = shaped_handle(kTiny, kVariants[1]);
  plipmi_handle h = eh.get();
  CHECK(strcmp(plipmi_device_name(h), "") == 0);
  REJECTS(plipmi_clone(h, nullptr), "null argument");
  REJECTS(plipmi_clone_resolution(h, 8, 64, 0, &out), "at least one patch");
  REJECTS(plipmi_clone_resolution(h, 64, 15, 0, &out), "at least one patch");
  REJECTS(plipmi_clone_resolution(h, 16 * 32, 16 * 32, 0, &out), "more than 1024 per sequence");
  REJECTS(plipmi_clone_resolution(h, 64, 64, -1, &out), "max_batch = -1");
  CHECK(out == nullptr);
  REJECTS(plipmi_encode_image(h, f, -1, f, 0, nullptr), "batch -1 outside [0, max_batch=8]");
  REJECTS(plipmi_encode_image(h, f, 9, f, 0, nullptr), "batch 9 outside");
  CHECK(plipmi_encode_image(h, nullptr, 0, nullptr, 0, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_encode_image(h, nullptr, 1, f, 0, nullptr), "null pixels/out");
  REJECTS(plipmi_encode_image(h, f, 1, nullptr, 0, nullptr), "null pixels/out");
  REJECTS(plipmi_encode_image_u8(h, u8, 9, f, 0, nullptr), "batch 9 outside");
  CHECK(plipmi_encode_image_u8(h, nullptr, 0, nullptr, 0, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_encode_image_u8(h, nullptr, 1, f, 0, nullptr), "null tiles/out");
  REJECTS(plipmi_encode_text(h, i64, nullptr, 9, 2, f, 0, nullptr), "batch 9 outside");
  CHECK(plipmi_encode_text(h, nullptr, nullptr, 0, 2, nullptr, 0, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_encode_text(h, nullptr, nullptr, 1, 2, f, 0, nullptr), "null ids/out");
  CHECK(plipmi_check_async(h) == PLIPMI_OK);
  int flag = 1;               // the device raises it; the next text call reports it once
  h->bad_id = &flag;
  CHECK(plipmi_check_async(h) == PLIPMI_ERR_TOKEN_ID && flag == 0 && err_has("outside [0, 512)"));
  CHECK(plipmi_check_async(h) == PLIPMI_OK);
  flag = 1;
  CHECK(plipmi_encode_text(h, i64, nullptr, 1, 2, f, 0, nullptr) == PLIPMI_ERR_TOKEN_ID);
  h->bad_id = nullptr;
  CHECK(plipmi_set_graph_batch(h, 100) == PLIPMI_OK && h->graph_batch == 8);
  CHECK(plipmi_set_graph_batch(h, -3) == PLIPMI_OK && h->graph_batch == 0);
  CHECK(plipmi_set_latency_batch(h, 8) == PLIPMI_OK && h->latency_batch == 8);
  CHECK(plipmi_set_latency_batch(h, -1) == PLIPMI_OK && h->latency_batch == 0);
  CHECK(plipmi_set_text_packing(h, 1) == PLIPMI_OK && h->text_pack);
  CHECK(plipmi_set_text_packing(h, 0) == PLIPMI_OK && !h->text_pack);
  CHECK(plipmi_get_pass_batch(h) == h->pass_batch);
  REJECTS(plipmi_streams_overlap(h, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_tower_shape(h, 0, nullptr), "null handle/shape");
  REJECTS(plipmi_tower_shape(h, 2, i32), "tower must be 0 (vision) or 1 (text), got 2");
  CHECK(plipmi_tower_shape(h, PLIPMI_VISION, i32) == PLIPMI_OK && i32[0] == 17 && i32[1] == 128 && i32[2] == 2 && i32[3] == 2);
  CHECK(plipmi_tower_shape(h, PLIPMI_TEXT, i32) == PLIPMI_OK && i32[0] == 16 && i32[1] == 128 && i32[2] == 2 && i32[3] == 2);
  REJECTS(plipmi_encode_tower_outputs(h, 0, f, nullptr, 9, 2, f, nullptr, nullptr, nullptr, nullptr), "batch 9 outside");
  REJECTS(plipmi_encode_tower_outputs(h, 5, f, nullptr, 1, 2, f, nullptr, nullptr, nullptr, nullptr), "got 5");
  CHECK(plipmi_encode_tower_outputs(h, 0, nullptr, nullptr, 0, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_encode_tower_outputs(h, 0, nullptr, nullptr, 1, 2, f, nullptr, nullptr, nullptr, nullptr), "null input");
  REJECTS(plipmi_encode_tower_outputs(h, 1, i64, nullptr, 1, 2, nullptr, nullptr, nullptr, nullptr, nullptr), "no output buffer given");
  REJECTS(plipmi_encode_tower_outputs(h, 0, f, i64, 1, 2, f, nullptr, nullptr, nullptr, nullptr), "takes no attention mask");
  REJECTS(plipmi_debug_hidden(h, 0, 0, f, 9, f, nullptr), "batch 9 outside");
  CHECK(plipmi_debug_hidden(h, 0, 0, nullptr, 0, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_debug_hidden(h, 0, 0, nullptr, 1, f, nullptr), "null input/out");
  REJECTS(plipmi_debug_hidden(h, 2, 0, f, 1, f, nullptr), "tower must be 0 or 1");
  REJECTS(plipmi_debug_hidden(h, 1, 3, i64, 1, f, nullptr), "layer 3 outside [0,2]");
  REJECTS(plipmi_debug_hidden(h, 0, -1, f, 1, f, nullptr), "layer -1 outside");
  REJECTS(plipmi_l2_normalize(h, nullptr, 1, 4, nullptr), "bad argument");
  REJECTS(plipmi_l2_normalize(h, f, 1, 0, nullptr), "bad argument");
  REJECTS(plipmi_logits(h, f, 1, f, 1, 0, 1.f, f, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_logits(h, f, 1, nullptr, 1, 4, 1.f, f, nullptr, nullptr, nullptr), "bad argument");
  CHECK(plipmi_logits(h, f, 0, f, 1, 4, 1.f, f, nullptr, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_topk(h, f, 1, 4, 5, i64, nullptr), "need 0 < k <= M");
  REJECTS(plipmi_topk(h, f, 1, 4, 0, i64, nullptr), "need 0 < k <= M");
  REJECTS(plipmi_resize_crop_u8(h, u8, 1, 0, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0, 4, u8, u8, nullptr), "bad argument");
  CHECK(plipmi_resize_crop_u8(h, nullptr, 0, 4, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0, 4, nullptr, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_resize_crop_u8(h, nullptr, 1, 4, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0, 4, u8, u8, nullptr), "null src/tmp/dst");
  REJECTS(plipmi_resize_crop_u8(h, u8, 1, 4, 4, 2, i32, nullptr, 1, 0, nullptr, nullptr, 0, 0, 0, 4, u8, u8, nullptr), "come in pairs");
  REJECTS(plipmi_resize_crop_u8(h, u8, 1, 4, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 2, 3, u8, u8, nullptr), "outside the 4-row image");
  REJECTS(plipmi_resize_crop_u8(h, u8, 1, 4, 4, 2, nullptr, nullptr, 0, 3, nullptr, nullptr, 0, 0, 0, 4, u8, u8, nullptr), "crop columns");
  REJECTS(plipmi_resize_crop_u8(h, u8, 1, 4, 4, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 3, 0, 4, u8, u8, nullptr), "crop rows");
  REJECTS(plipmi_resize_crop_u8_ragged(h, u8, 8, i64, i32, i64, i32, 1, 2, 2, 4, u8, 8, u8, nullptr), "bad argument");
  CHECK(plipmi_resize_crop_u8_ragged(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 2, 0, 4, nullptr, 0, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_resize_crop_u8_ragged(h, u8, 8, i64, i32, i64, i32, kRaggedMaxBatch + 1, 2, 0, 4, u8, 8, u8, nullptr), "images in one call");
  REJECTS(plipmi_resize_crop_u8_ragged(h, u8, 8, i64, i32, i64, nullptr, 1, 2, 0, 4, u8, 8, u8, nullptr), "null src/offsets/hw/workspace/dst");
  {
    const int32_t hw[4] = {40, 60, 32, 32};
    const int64_t off[2] = {0, 40 * 60 * 3};
    const size_t src_bytes = 40 * 60 * 3 + 32 * 32 * 3;
    REJECTS(plipmi_resize_crop_u8_ragged(h, u8, src_bytes - 1, i64, i32, off, hw, 2, 16, 0, 64, u8, 8, u8, nullptr), "image 1 (32 x 32");
    REJECTS(plipmi_resize_crop_u8_ragged(h, u8, src_bytes, i64, i32, off, hw, 2, 16, 0, 1, u8, 8, u8, nullptr), "taps of the batch's largest scale");
    REJECTS(plipmi_resize_crop_u8_ragged(h, u8, src_bytes, i64, i32, off, hw, 2, 16, 0, 64, u8, 8, u8, nullptr), "plipmi_resize_ragged_workspace asks for");
    // plipmi_resize_ragged_workspace: 0 for what it cannot size, else the layout's total -- which grows with the batch
    CHECK(plipmi_resize_ragged_workspace(nullptr, 2, 16, 64) == 0);
    CHECK(plipmi_resize_ragged_workspace(hw, 0, 16, 64) == 0);
    CHECK(plipmi_resize_ragged_workspace(hw, 2, 0, 64) == 0);
    CHECK(plipmi_resize_ragged_workspace(hw, 2, 16, 0) == 0);
    const size_t one = plipmi_resize_ragged_workspace(hw, 1, 16, 64), two = plipmi_resize_ragged_workspace(hw, 2, 16, 64);
    CHECK(one > 0 && two > one && two % 256 == 0);
    CHECK(two == rr_layout(hw, 2, 16, 64).total);
  }
  REJECTS(plipmi_similarity_topk(h, f, 1, f, 0, 32, 1, i64, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_similarity_topk(h, nullptr, 1, f, 4, 32, 1, i64, nullptr, nullptr), "null keys/space/idx");
  REJECTS(plipmi_similarity_topk(h, f, 1, f, 4, 32, 5, i64, nullptr, nullptr), "need 0 < k <= min(Ns, 1024)");
  REJECTS(plipmi_similarity_topk(h, f, 1, f, 4, 48, 1, i64, nullptr, nullptr), "multiple of 32");
  CHECK(plipmi_similarity_topk(h, nullptr, 0, nullptr, 4, 32, 1, nullptr, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_probe_fit(h, nullptr, 4, 4, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "null handle / X / WB");
  REJECTS(plipmi_probe_fit(h, x16, 0, 4, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "need N > 0");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, i32, 0, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "problems, got 0");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, i32, PLIPMI_PROBE_MAX_K + 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "problems, got");
  REJECTS(plipmi_probe_fit(h, x16, 4, 6, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "embedding width 6 unsupported");
  REJECTS(plipmi_probe_fit(h, x16, 4, 1028, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "embedding width 1028 unsupported");
  REJECTS(plipmi_probe_fit(h, x16 + 1, 4, 4, i32, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "16-byte aligned");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, nullptr, 1, f, f, 1.f, 10, 1e-4f, f, &info, nullptr), "null y / pos_w / neg_w");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, i32, 1, f, f, 0.f, 10, 1e-4f, f, &info, nullptr), "alpha must be finite");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, i32, 1, f, f, 1.f, 0, 1e-4f, f, &info, nullptr), "max_iter >= 1");
  REJECTS(plipmi_probe_fit(h, x16, 4, 4, i32, 1, f, f, 1.f, 10, -1.f, f, &info, nullptr), "max_iter >= 1");
  REJECTS(plipmi_probe_predict(h, x16, 4, 4, f, 1, nullptr, nullptr, nullptr), "null pred");
  REJECTS(plipmi_probe_loss_grad(h, x16, 4, 4, i32, 1, f, f, 1.f, f, nullptr, f, nullptr), "null loss_out / grad_out");
  CHECK(plipmi_profile_enable(h, 1) == PLIPMI_OK && h->prof.on);
  CHECK(plipmi_profile_enable(h, 0) == PLIPMI_OK && !h->prof.on);
  REJECTS(plipmi_profile_read(h, rows, 0, &n), "bad argument");
  {  // packing is a mode of the pooled last block
    auto dense = shaped_handle(kTiny, kVariants[2]);
    REJECTS(plipmi_set_text_packing(dense.get(), 1), "caption packing needs");
    CHECK(plipmi_set_text_packing(dense.get(), 0) == PLIPMI_OK);
    auto f32 = shaped_handle(kTiny, kVariants[0]);
    CHECK(plipmi_set_latency_batch(f32.get(), 8) == PLIPMI_OK && f32->latency_batch == 0);   // a 16-bit engine's path
  }

  // kernel-level entries (plipmi_test.h): their argument checks
  REJECTS(plipmi_gemm_nt(3, 0, -1, 4, 4, 4, f, f, f, 1.f, f, nullptr), "bad dtype");
  REJECTS(plipmi_gemm_nt(0, 4, -1, 4, 4, 4, f, f, f, 1.f, f, nullptr), "epilogue must be 0..3");
  REJECTS(plipmi_gemm_nt(0, 0, -1, 4, 0, 4, f, f, f, 1.f, f, nullptr), "bad shape / null pointer");
  REJECTS(plipmi_gemm_nt(0, 0, -1, 4, 4, 4, f, nullptr, f, 1.f, f, nullptr), "bad shape / null pointer");
  REJECTS(plipmi_gemm_nt(0, 0, -1, 4, 4, 4, f, f, nullptr, 1.f, f, nullptr), "bias required");
  REJECTS(plipmi_gemm_nt_traced(-1, 0, -1, 4, 4, 4, f, f, f, 1.f, f, nullptr, nullptr), "bad dtype");
  REJECTS(plipmi_gemm_nt_ld(3, 0, -1, 4, 4, 4, f, 4, f, 4, f, 1.f, f, nullptr), "bad dtype");
  REJECTS(plipmi_gemm_nt_ld(0, -1, -1, 4, 4, 4, f, 4, f, 4, f, 1.f, f, nullptr), "epilogue must be 0..3");
  REJECTS(plipmi_gemm_nt_ld(0, 0, -1, 4, 4, 4, f, 3, f, 4, f, 1.f, f, nullptr), "leading dimension");
  REJECTS(plipmi_gemm_nt_ld(1, 0, -1, 4, 4, 8, f, 12, f, 8, f, 1.f, f, nullptr), "leading dimension");
  REJECTS(plipmi_gemm_nt_ld(0, 0, -1, 4, 4, 4, f, 4, f, 4, nullptr, 1.f, f, nullptr), "bias required");
  REJECTS(plipmi_gemm_nt_ln(0, 0, -1, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, nullptr), "16-bit-engine forms");
  REJECTS(plipmi_gemm_nt_ln(1, 5, -1, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, nullptr), "bad argument");
  REJECTS(plipmi_gemm_nt_ln(1, 0, -1, 4, 128, 128, f, f, f, nullptr, 2, 1e-5f, f, f, f, nullptr), "need the row statistics");
  REJECTS(plipmi_gemm_nt_ln(1, 1, -1, 4, 128, 128, f, f, f, f, 3, 1e-5f, f, f, f, nullptr), "must be even");
  REJECTS(plipmi_gemm_nt_ln(1, 2, -1, 4, 96, 128, f, f, f, f, 2, 1e-5f, f, f, f, nullptr), "need xb_out, st_out");
  REJECTS(plipmi_gemm_nt_ln(2, 4, -3, 4, 128, 256, f, f, f, f, 2, 1e-5f, f, f, f, nullptr), "the engine re-codes them in enter_block");
  REJECTS(plipmi_attention(3, 0, f, f, 1, 4, 1, 0, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_attention(0, 0, f, nullptr, 1, 4, 1, 0, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_attention_probs(0, f, f, 1, 1025, 1, 0, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_attention_probs(4, f, f, 1, 4, 1, 0, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_qkv_attention(1, nullptr, f, f, f, 2, 1e-5f, f, 1, 77, 2, 1, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_qkv_attention(1, f, f, f, f, 3, 1e-5f, f, 1, 77, 2, 1, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_qkv_attention(0, f, f, f, f, 2, 1e-5f, f, 1, 77, 2, 1, nullptr, nullptr, nullptr), "takes 16-bit operands");
  REJECTS(plipmi_qkv_attention(1, f, f, f, f, 2, 1e-5f, f, 1, 16, 2, 1, nullptr, nullptr, nullptr), "65 .. 80 tokens");
  REJECTS(plipmi_resample_pos(f, f, 2, 2, 2, 4, nullptr), "distinct");
  REJECTS(plipmi_resample_pos(f, f + 1, 0, 2, 2, 4, nullptr), "bad argument");
  REJECTS(plipmi_resize_ragged_tables(0, 4, 0, 4, 8, i32, i32, nullptr), "bad argument");
  REJECTS(plipmi_resize_ragged_tables(8, 4, 2, 3, 8, i32, i32, nullptr), "bad argument");
  REJECTS(plipmi_resize_ragged_tables(4 * (kRaggedMaxRatio + 1), 4, 0, 4, 1024, i32, i32, nullptr), "in / out above");
  REJECTS(plipmi_resize_ragged_tables(8, 4, 0, 4, 1, i32, i32, nullptr), "taps");
  CHECK(plipmi_resize_ragged_tables(8, 4, 0, 0, 64, nullptr, nullptr, nullptr) == PLIPMI_OK);
  REJECTS(plipmi_resize_ragged_tables(8, 4, 0, 4, 64, nullptr, i32, nullptr), "null bounds/coef");
  REJECTS(plipmi_layernorm(f, 4, f, f, f + 4, 3, 1, 4, 1e-5f, nullptr), "bad argument");
  REJECTS(plipmi_layernorm(f, 4, f, f, f + 4, 0, 1, 6, 1e-5f, nullptr), "LayerNorm width 6");
  REJECTS(plipmi_layernorm(f, 2, f, f, f + 4, 0, 1, 4, 1e-5f, nullptr), "row stride 2");
  REJECTS(plipmi_layernorm(f, 4, f, f, f, 1, 1, 4, 1e-5f, nullptr), "in place");
  REJECTS(plipmi_layernorm_emit(0, f, f, f, f, f, f, 1, 64, 1e-5f, nullptr), "bad argument");
  REJECTS(plipmi_layernorm_emit(1, f, f, f, f, f, f, 1, 96, 1e-5f, nullptr), "width 96");
  REJECTS(plipmi_fold_ln(0, f, f, f, f, f, f, 1, 4, 1.f, nullptr), "16-bit dtype");
  REJECTS(plipmi_fold_ln(1, f, f, f, f, f, f, 1, 6, 1.f, nullptr), "16-bit dtype");
  REJECTS(plipmi_text_embed_emit(0, 0, i64, f, f, f, f, f, 1, 4, 64, 8, 2, i32, i32, i32, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_text_embed_emit(1, 2, i64, f, f, f, f, f, 1, 4, 64, 8, 2, i32, i32, i32, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_text_embed_emit(1, 0, i64, f, f, f, f, f, 1, 4, 96, 8, 2, i32, i32, i32, nullptr, nullptr), "width 96");
  REJECTS(plipmi_text_embed_emit(1, 1, i64, f, f, f, f, f, 1, 4, 64, 8, 2, nullptr, i32, i32, nullptr, nullptr), "the packed form returns");
  REJECTS(plipmi_text_embed_emit(1, 1, i64, f, f, f, f, f, 1, 257, 64, 8, 2, i32, i32, i32, nullptr, nullptr), "packing: S <= 256");
  REJECTS(plipmi_pool_rows(2, f, 1, 4, 4, nullptr, -1, f, f, 1e-5f, f, 4, 0, f, nullptr), "bad argument");
  REJECTS(plipmi_pool_rows(0, f, 1, 4, 4, nullptr, -1, f, f, 1e-5f, nullptr, 4, 0, f, nullptr), "pooled head");
  REJECTS(plipmi_pool_rows(0, f, 1, 4, 4, nullptr, -1, f, f, 1e-5f, f, 1025, 0, f, nullptr), "pooled head");
  REJECTS(plipmi_pool_rows(1, f, 1, 4, 6, nullptr, -1, f, f, 1e-5f, nullptr, 0, 0, f, nullptr), "pooled LayerNorm");
  REJECTS(plipmi_pool_gather(0, f, f, f, 1, 4, 8, nullptr, -1, nullptr, f, f, nullptr), "16-bit dtype");
  REJECTS(plipmi_pool_gather(1, f, f, f, 1, 4, 12, nullptr, -1, nullptr, f, f, nullptr), "16-bit dtype");
  REJECTS(plipmi_head_gemm(f, f, f, 1, 48, 32, 1.f, nullptr), "N % 32 == 0");
  REJECTS(plipmi_head_gemm(nullptr, f, f, 1, 32, 32, 1.f, nullptr), "N % 32 == 0");
  REJECTS(plipmi_recode_planes(nullptr, f, 1, 8, 1, 2, nullptr), "null planes");
  REJECTS(plipmi_recode_planes(f, f, 1, 12, 1, 2, nullptr), "null planes");
  // the vision front end and the packed-row mechanisms
  REJECTS(plipmi_unfold_patches(3, 0, x16, x16, 1, 16, 16, 16, 768, nullptr), "bad argument");
  REJECTS(plipmi_unfold_patches(0, 2, x16, x16, 1, 16, 16, 16, 768, nullptr), "bad argument");
  REJECTS(plipmi_unfold_patches(0, 0, nullptr, x16, 1, 16, 16, 16, 768, nullptr), "bad argument");
  REJECTS(plipmi_unfold_patches(0, 0, x16, x16, 1, 16, 15, 16, 768, nullptr), "at least one patch");
  REJECTS(plipmi_unfold_patches(0, 0, x16, x16, 1, 16, 16, 0, 768, nullptr), "1 <= patch <= 64");
  REJECTS(plipmi_unfold_patches(1, 0, x16, x16, 1, 16, 16, 16, 764, nullptr), "Kpad 764");
  REJECTS(plipmi_unfold_patches(1, 1, x16, x16, 1, 15, 15, 15, 678, nullptr), "Kpad 678");
  REJECTS(plipmi_unfold_patches(0, 0, x16 + 1, x16, 1, 16, 16, 16, 768, nullptr), "16-byte aligned");
  REJECTS(plipmi_cls_rows(nullptr, x16, x16, 1, 2, 4, nullptr), "bad argument");
  REJECTS(plipmi_cls_rows(x16, x16, x16, 1, 0, 4, nullptr), "tokens >= 1");
  REJECTS(plipmi_cls_rows(x16, x16, x16, 1, 2, 6, nullptr), "D % 4 == 0");
  REJECTS(plipmi_cls_rows(x16, x16 + 1, x16, 1, 2, 4, nullptr), "16-byte aligned");
  REJECTS(plipmi_gemm_patch(3, -1, 4, 4, 4, f, 4, f, 4, f, 2, f, nullptr), "bad dtype");
  REJECTS(plipmi_gemm_patch(0, -1, 4, 6, 4, f, 4, f, 4, f, 2, f, nullptr), "leading dimension");
  REJECTS(plipmi_gemm_patch(0, -1, 4, 4, 4, f, 3, f, 4, f, 2, f, nullptr), "leading dimension");
  REJECTS(plipmi_gemm_patch(1, -1, 4, 4, 8, f, 8, f, 12, f, 2, f, nullptr), "leading dimension");
  REJECTS(plipmi_gemm_patch(0, -1, 4, 4, 4, f, 4, f, 4, nullptr, 2, f, nullptr), "null pointer");
  REJECTS(plipmi_gemm_patch(0, -1, 4, 4, 4, f, 4, f, 4, f, 0, f, nullptr), "np = 0");
  REJECTS(plipmi_gemm_patch(0, -1, 4, 4, 4, f, 4, f, 4, f, 3, f, nullptr), "np = 3");
  REJECTS(plipmi_gemm_patch(0, -3, 4, 64, 256, f, 256, f, 256, f, 2, f, nullptr), "variant -3: the small-M kernel takes 16-bit operands");
  REJECTS(plipmi_gemm_patch(1, -3, 4, 64, 640, f, 640, f, 640, f, 2, f, nullptr), "K % 256 == 0");      // Kpad of a 14-pixel patch
  REJECTS(plipmi_gemm_patch(2, -3, 4, 32, 256, f, 256, f, 256, f, 2, f, nullptr), "N % 64 == 0");
  REJECTS(plipmi_gemm_patch(1, -4, 4, 64, 256, f, 256, f, 256, f, 2, f, nullptr), "variant -4");
  REJECTS(plipmi_gemm_patch_gather(0, f, nullptr, f, f, f, 1, 16, 16, 16, 256, nullptr), "16-bit-engine form");
  REJECTS(plipmi_gemm_patch_gather(1, nullptr, nullptr, f, f, f, 1, 16, 16, 16, 256, nullptr), "exactly one of pixels / tiles");
  REJECTS(plipmi_gemm_patch_gather(1, f, u8, f, f, f, 1, 16, 16, 16, 256, nullptr), "exactly one of pixels / tiles");
  REJECTS(plipmi_gemm_patch_gather(1, f, nullptr, nullptr, f, f, 1, 16, 16, 16, 256, nullptr), "exactly one of pixels / tiles");
  REJECTS(plipmi_gemm_patch_gather(2, f, nullptr, f, f, f, 1, 28, 28, 14, 256, nullptr), "patch 14");
  REJECTS(plipmi_gemm_patch_gather(1, f, nullptr, f, f, f, 1, 48, 50, 16, 256, nullptr), "width % 4 == 0");
  REJECTS(plipmi_gemm_patch_gather(1, nullptr, u8, f, f, f, 1, 15, 16, 16, 256, nullptr), "at least one patch");
  REJECTS(plipmi_gemm_patch_gather(1, f, nullptr, f, f, f, 1, 16, 16, 16, 128, nullptr), "whole 256-column tiles");
  REJECTS(plipmi_gemm_patch_gather(1, f, nullptr, f, f, f, 400, 1024, 1024, 16, 256, nullptr), "below 4 GiB");
  REJECTS(plipmi_gemm_nt_ln_rows(1, 0, -1, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, nullptr, nullptr), "null m_dev");
  REJECTS(plipmi_gemm_nt_ln_rows(1, 0, -2, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, i32, nullptr), "variant -2 does not read");
  REJECTS(plipmi_gemm_nt_ln_rows(2, 0, -3, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, i32, nullptr), "variant -3 does not read");
  REJECTS(plipmi_gemm_nt_ln_rows(0, 0, -1, 4, 128, 128, f, f, f, f, 2, 1e-5f, f, f, f, i32, nullptr), "16-bit-engine forms");
  REJECTS(plipmi_gemm_nt_ln_rows(1, 1, 0, 4, 128, 128, f, f, f, f, 3, 1e-5f, f, f, f, i32, nullptr), "must be even");
  REJECTS(plipmi_attention_packed(0, 1, f, f, 1, 4, 1, 0, nullptr, i32, nullptr), "bad argument");
  REJECTS(plipmi_attention_packed(1, 1, f, f, 1, 4, 1, 0, nullptr, nullptr, nullptr), "bad argument");
  REJECTS(plipmi_attention_packed(1, 0, f, f, 1, 4, 1, 0, nullptr, i32, nullptr), "impl 1, S <= 128 (got impl 0");
  REJECTS(plipmi_attention_packed(2, 1, f, f, 1, 129, 1, 1, nullptr, i32, nullptr), "S=129");
  CHECK(plipmi_gemm_variant_built(3, 0) == 0 && plipmi_gemm_variant_built(-1, 0) == 0);
  CHECK(plipmi_gemm_variant_name(-1) == nullptr && plipmi_gemm_variant_name(1 << 20) == nullptr);
  CHECK(plipmi_gemm_variant_name(0) != nullptr && strlen(plipmi_gemm_variant_name(0)) > 0);
}

// ---- the process-wide hooks: in range they take effect and move the epoch, out of range they change nothing --------------------
static void check_hooks() {
  int n_variants = 0;
  while (plipmi_gemm_variant_name(n_variants)) ++n_variants;
  CHECK(n_variants > 0);
  unsigned epoch = g_hook_epoch;
  REJECTS(plipmi_test_force_gemm_tile(n_variants), "tile");
  REJECTS(plipmi_test_force_gemm_tile(-3), "tile");
  REJECTS(plipmi_test_remap_gemm_tile(n_variants, 0), "remap");
  REJECTS(plipmi_test_remap_gemm_tile(0, n_variants), "remap");
  REJECTS(plipmi_test_remap_gemm_tile(-1, 0), "remap");
  REJECTS(plipmi_test_fused_qkv_attention(3), "fused q/k/v + attention mode 3");
  REJECTS(plipmi_test_fused_qkv_attention(-1), "fused q/k/v + attention mode -1");
  REJECTS(plipmi_test_patch_gather(2), "patch gather 2");
  REJECTS(plipmi_test_patch_gather(-1), "patch gather -1");
  CHECK(g_hook_epoch == epoch && g_fuse_qkv_attention == 1 && g_patch_gather == 1);
  CHECK(plipmi_test_force_gemm_tile(0) == PLIPMI_OK && g_hook_epoch == ++epoch);
  CHECK(plipmi_test_force_gemm_tile(-2) == PLIPMI_OK && g_hook_epoch == ++epoch);
  CHECK(plipmi_test_force_gemm_tile(-1) == PLIPMI_OK && g_hook_epoch == ++epoch);
  CHECK(plipmi_test_remap_gemm_tile(0, n_variants - 1) == PLIPMI_OK && g_hook_epoch == ++epoch);
  CHECK(plipmi_test_remap_gemm_tile(0, -1) == PLIPMI_OK && g_hook_epoch == ++epoch);
  for (int mode = 0; mode <= 2; ++mode) CHECK(plipmi_test_fused_qkv_attention(mode) == PLIPMI_OK && g_fuse_qkv_attention == mode && g_hook_epoch == ++epoch);
  for (int on = 0; on <= 1; ++on) CHECK(plipmi_test_patch_gather(on) == PLIPMI_OK && g_patch_gather == on && g_hook_epoch == ++epoch);
  plipmi_test_fused_qkv_attention(0);
  plipmi_test_patch_gather(0);
  epoch += 2;
  plipmi_test_reset_hooks();
  CHECK(g_fuse_qkv_attention == 1 && g_patch_gather == 1 && g_hook_epoch == ++epoch);
}

// ---- pass arithmetic: the passes of a call cover its batch in equal parts ---------------------------------------------------
static void check_passes() {
  for (int pass_batch : {0, 32, 256})
    for (int B = 1; B <= 2048; ++B) {
      const int n = passes_of(pass_batch, B);
      int sum = 0, lo = B, hi = 0;
      for (int i = 0; i < n; ++i) {
        const int r = pass_rows(B, n, i);
        sum += r; lo = std::min(lo, r); hi = std::max(hi, r);
      }
      const bool split = pass_batch > 0 && B >= 2 * pass_batch;
      if (n < 1 || sum != B || hi - lo > 1 || lo < 1 || (n > 1) != split || (split && hi > pass_batch)) {
        ++g_failed;
        printf("FAILED passes: pass_batch %d B %d -> %d passes, rows sum %d, min %d max %d\n", pass_batch, B, n, sum, lo, hi);
        return;
      }
    }
}

// ---- two-pass carving ------------------------------------------------------------------------------------------------------
struct Region { size_t off, bytes; };
struct RecordingCarver : Carver {   // the product's Carver, with every region it hands out written down
  std::vector<Region> regions;
  template <typename T> T* take(size_t count, size_t elem) {
    T* p = Carver::take<T>(count, elem);
    regions.push_back({off - count * elem, count * elem});
    return p;
  }
};
// carve(sizing) then carve(placing) over a host allocation of exactly the sized bytes; every region is written to its full size,
// so a region carved too small (or a slab sized short) is a heap-buffer-overflow under AddressSanitizer.  Returns the slab's bytes.
template <typename Carve>
static size_t check_carving(const char* what, Carve&& carve) {
  RecordingCarver sizing;
  carve(sizing);
  const size_t bytes = align_up(sizing.off, 256);
  char* slab = static_cast<char*>(malloc(bytes));
  RecordingCarver placing;
  placing.base = slab;
  carve(placing);
  bool ok = slab != nullptr && placing.off == sizing.off && placing.regions.size() == sizing.regions.size() && !placing.regions.empty();
  size_t end = 0;
  for (size_t i = 0; ok && i < placing.regions.size(); ++i) {
    const Region& r = placing.regions[i];
    ok = r.off == sizing.regions[i].off && r.bytes == sizing.regions[i].bytes   // the two passes agree region by region
         && r.off % 256 == 0 && r.off >= end                                    // aligned, and behind its predecessor: no overlap
         && r.off + r.bytes <= bytes;                                            // inside the slab
    end = r.off + r.bytes;
    if (ok) memset(slab + r.off, 0x5a, r.bytes);
  }
  if (!ok) { ++g_failed; printf("FAILED carving: %s (%zu regions, %zu bytes)\n", what, placing.regions.size(), bytes); }
  free(slab);
  return bytes;
}

static void check_pointer(const char* what, const void* p, const char* base, size_t bytes, bool expected) {
  const char* c = static_cast<const char*>(p);
  const bool ok = expected ? (c != nullptr && (c - base) % 256 == 0 && c >= base && c < base + bytes) : c == nullptr;
  if (!ok) { ++g_failed; printf("FAILED pointer %s: %s\n", what, expected ? "not an aligned address inside the slab" : "set although its mode is off"); }
}

static void check_shapes_and_carving() {
  const Arch* archs[] = {&kTiny, &kVitB32, &kVitL14_336};
  for (const Arch* a : archs)
    for (size_t vi = 0; vi < 4; ++vi) {
      const Variant& v = kVariants[vi];
      std::string what = std::string(a->name) + " / " + v.name;
      std::shared_ptr<Model> m;
      auto e = shaped_handle(*a, v, &m);
      // shape resolution
      const int grid = a->image / a->patch;
      CHECK(e->img_h == a->image && e->img_w == a->image && e->gh == grid && e->gw == grid && e->np == grid * grid);
      CHECK(e->vis.S == grid * grid + 1 && e->txt.S == a->ctx && e->max_batch == a->max_batch);
      CHECK(e->graph_batch_cap == std::min(a->max_batch, 32) && e->graph_batch == e->graph_batch_cap);
      CHECK(m->half() == (v.dtype != PLIPMI_F32) && m->esz == (m->half() ? 2u : 4u));
      CHECK(m->ln_fold == (vi == 1 || vi == 2) && m->pooled_last == (vi == 1));
      CHECK(e->attn_impl_vis == (m->half() ? 1 : 0) && e->attn_impl_txt == e->attn_impl_vis);
      CHECK(m->kpad % 64 == 0 && m->kpad >= 3 * a->patch * a->patch && m->kpad < 3 * a->patch * a->patch + 64);
      CHECK(e->pass_batch == 0 || (e->pass_batch >= 256 && e->pass_batch % 32 == 0));
      CHECK(!e->text_pack && e->latency_batch == 0);
      // carving: the model's weights, the handle's workspace
      const size_t wbytes = check_carving((what + " weights").c_str(), [&](RecordingCarver& c) { carve_weights(m.get(), c); });
      const size_t sbytes = check_carving((what + " workspace").c_str(), [&](RecordingCarver& c) { carve_workspace(e.get(), c); });
      if (a == &kTiny) {
        CHECK(sbytes == kTinyCloneSlab[vi]);
        CHECK(wbytes + sbytes == kTinyCreateSlab[vi]);
      }
      // the pointers the handle keeps: placed over a fake base (never dereferenced), each inside the slab where its mode is on
      char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);
      Carver placing;
      placing.base = base;
      carve_workspace(e.get(), placing);
      for (const Tower* t : {&e->vis, &e->txt}) {
        check_pointer("pooled", t->pooled, base, sbytes, true);
        check_pointer("x", t->x, base, sbytes, true);       check_pointer("h", t->h, base, sbytes, true);
        check_pointer("qkv", t->qkv, base, sbytes, true);   check_pointer("att", t->att, base, sbytes, true);
        check_pointer("mlp", t->mlp, base, sbytes, true);
        check_pointer("st", t->st, base, sbytes, m->ln_fold); check_pointer("lo", t->lo, base, sbytes, m->ln_fold);
        check_pointer("cu", t->cu, base, sbytes, m->ln_fold && t == &e->txt);
        check_pointer("rowmap", t->rowmap, base, sbytes, m->ln_fold && t == &e->txt);
        check_pointer("mdev", t->mdev, base, sbytes, m->ln_fold && t == &e->txt);
        check_pointer("xp", t->xp, base, sbytes, m->pooled_last);     check_pointer("attp", t->attp, base, sbytes, m->pooled_last);
        check_pointer("hp", t->hp, base, sbytes, m->pooled_last);     check_pointer("mlpp", t->mlpp, base, sbytes, m->pooled_last);
        check_pointer("stp", t->stp, base, sbytes, m->pooled_last);
      }
      check_pointer("patches", e->patches, base, sbytes, true);
      check_pointer("g_vin", e->g_vin, base, sbytes, true);   check_pointer("g_tin", e->g_tin, base, sbytes, true);
      check_pointer("g_tmask", e->g_tmask, base, sbytes, true);
      check_pointer("g_vout", e->g_vout, base, sbytes, true); check_pointer("g_tout", e->g_tout, base, sbytes, true);
    }
  // one derived resolution: 288 x 256 on ViT-B/32, the batch derived from the source's workspace
  {
    auto src = shaped_handle(kVitB32, kVariants[1]);
    int B = 0;
    CHECK(check_resolution(src.get(), 288, 256, 0, &B) == PLIPMI_OK);
    CHECK(B == 256 * 50 / 73);                       // 9 x 8 patches + CLS = 73 tokens
    auto e = std::make_unique<plipmi_engine>(src->model);
    shape_handle(e.get(), B, 288, 256);
    CHECK(e->gh == 9 && e->gw == 8 && e->np == 72 && e->vis.S == 73 && e->img_h == 288 && e->img_w == 256 && e->max_batch == B);
    CHECK(e->graph_batch_cap == 32 && e->txt.S == 77);
    check_carving("ViT-B/32 at 288 x 256 workspace", [&](RecordingCarver& c) { carve_workspace(e.get(), c); });
    int B1 = 0;
    CHECK(check_resolution(src.get(), 295, 271, 5, &B1) == PLIPMI_OK && B1 == 5);   // the grid floors: still 9 x 8
    auto e1 = std::make_unique<plipmi_engine>(src->model);
    shape_handle(e1.get(), B1, 295, 271);
    CHECK(e1->gh == 9 && e1->gw == 8 && e1->graph_batch_cap == 5 && e1->graph_batch == 5);
    check_carving("ViT-B/32 at 295 x 271, max_batch 5, workspace", [&](RecordingCarver& c) { carve_workspace(e1.get(), c); });
  }
}

int main() {
  check_create_validation();
  check_early_returns();
  check_hooks();
  check_passes();
  check_shapes_and_carving();
  if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
  printf("host checks passed\n");
  return 0;
}
