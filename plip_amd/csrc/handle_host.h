// handle_host.h -- the HIP-free half of building a handle: config validation, the model's and the handle's shape facts, the
// per-handle settings that follow from them, the pass arithmetic and the two-pass slab carving.  Plain C++: nothing here calls a
// HIP function, so tests/native/host_checks.hip drives it under AddressSanitizer on a machine without a GPU.
#pragma once
#include <stddef.h>

#include <algorithm>

#include "handle.h"

#ifndef PLIPMI_DEFAULT_ATTENTION
#define PLIPMI_DEFAULT_ATTENTION 1
#endif

namespace plipmi {

// Batches of at most this many samples take the latency path (split-K small-M GEMMs) -- 0: nobody does unless the caller asks
// (plipmi_set_latency_batch).  It is faster up to batch 8 (pair latency 1.16 -> 0.79 ms at batch 1, 1.32 -> 1.09 ms at 8;
// slower from 16 on: profiles/r04_small_batch_latency.txt), but its other summation order moves the 16-bit activations'
// roundings: embeddings of the two regimes differ by up to 6e-4, and by default a row's embedding is the same bits whatever
// batch it arrives in -- which the host loops' coalescing (plip_amd/plip.py) and the caches' consumers rely on.
constexpr int kLatencyBatch = 0;

// plipmi_create's argument checks up to the first HIP call.  *g = the caller's config read at the caller's size.
inline int validate_config(const plipmi_config* cfg, plipmi_config* g_out) {
  // The caller's struct may be OLDER (shorter) than this library's: read what it has, later members are 0 = their defaults
  // (a member appended at the tail used to be read as garbage from a caller compiled against the previous header).
  const size_t kMinSize = offsetof(plipmi_config, max_batch) + sizeof(int32_t);   // the members every version has had
  if (cfg->struct_size < (int)kMinSize || cfg->struct_size > (int)sizeof(plipmi_config))
    return fail(PLIPMI_ERR_INVALID, "plipmi_config.struct_size = %d: expected sizeof(plipmi_config) of the caller's header, %zu .. %zu "
                "(this library: version %d)", cfg->struct_size, kMinSize, sizeof(plipmi_config), PLIPMI_VERSION);
  memset(g_out, 0, sizeof(*g_out));
  memcpy(g_out, cfg, (size_t)cfg->struct_size);
  g_out->struct_size = (int32_t)sizeof(plipmi_config);
  const plipmi_config& g = *g_out;
  if (!valid_dtype(g.compute_dtype))
    return fail(PLIPMI_ERR_INVALID, "compute_dtype must be PLIPMI_F32, PLIPMI_BF16 or PLIPMI_F16");
  if (g.flags & ~(PLIPMI_FLAG_SEPARATE_LAYERNORM | PLIPMI_FLAG_DENSE_LAST_BLOCK | PLIPMI_FLAG_PACK_CAPTIONS | PLIPMI_FLAG_VALU_ATTENTION |
                  PLIPMI_FLAG_TEXT_TOWER_F16 | PLIPMI_FLAG_VISION_GELU | PLIPMI_FLAG_TEXT_GELU))
    return fail(PLIPMI_ERR_INVALID, "unknown bits in plipmi_config.flags (0x%x)", (unsigned)g.flags);
  if ((g.flags & PLIPMI_FLAG_TEXT_TOWER_F16) && g.compute_dtype != PLIPMI_BF16)
    return fail(PLIPMI_ERR_INVALID, "PLIPMI_FLAG_TEXT_TOWER_F16 is a mode of the bf16 engine (compute_dtype PLIPMI_BF16)");
  if (g.text_f16_layers < 0 || g.text_f16_layers > g.t_layers || (g.text_f16_layers > 0 && g.compute_dtype != PLIPMI_BF16))
    return fail(PLIPMI_ERR_INVALID, "text_f16_layers = %d: 0 .. t_layers leading text blocks, bf16 engine only", g.text_f16_layers);
  // head_dim = width / heads, per tower: 64 (the kernels every OpenAI CLIP / PLIP variant runs), or another multiple of 8 up to 128
  // (the padded-head attention kernels: ViT-H/14's vision heads are 80 wide, ViT-g/14's 88) -- a text tower up to 120: no published
  // CLIP has a wider text head
  auto head_ok = [](int width, int heads, int max_head) {
    return heads > 0 && width > 0 && width % heads == 0 && width / heads % 8 == 0 && width / heads >= 64 && width / heads <= max_head;
  };
  if (!head_ok(g.v_width, g.v_heads, 128) || !head_ok(g.t_width, g.t_heads, 120))
    return fail(PLIPMI_ERR_INVALID, "head_dim = width / heads must be a multiple of 8, 64 .. 128 (vision) / 64 .. 120 (text) "
                "(v_width=%d/%d heads, t_width=%d/%d heads)", g.v_width, g.v_heads, g.t_width, g.t_heads);
  if ((g.flags & PLIPMI_FLAG_PACK_CAPTIONS) && g.t_width != g.t_heads * 64)
    return fail(PLIPMI_ERR_INVALID, "PLIPMI_FLAG_PACK_CAPTIONS needs a text tower with head_dim 64: packed rows are a form of the head-64 "
                "short-sequence attention kernel (t_width=%d/%d heads)", g.t_width, g.t_heads);
  if (g.patch_size <= 0 || g.image_size % g.patch_size) return fail(PLIPMI_ERR_INVALID, "image_size %% patch_size != 0");
  if (g.v_width % 128 || g.v_mlp % 128 || g.t_width % 128 || g.t_mlp % 128)
    return fail(PLIPMI_ERR_INVALID, "widths and MLP sizes must be multiples of 128 (GEMM tile)");
  if (g.v_width > 2048 || g.t_width > 2048 || g.projection_dim > 1024 || g.projection_dim <= 0)
    return fail(PLIPMI_ERR_INVALID, "width > 2048 or projection_dim > 1024 not supported");
  if (g.max_batch <= 0 || g.v_layers <= 0 || g.t_layers <= 0 || g.context_length <= 0 || g.vocab_size <= 0)
    return fail(PLIPMI_ERR_INVALID, "non-positive size in config");
  const int tokens = (g.image_size / g.patch_size) * (g.image_size / g.patch_size) + 1;
  if (tokens > 1024 || g.context_length > 1024) return fail(PLIPMI_ERR_INVALID, "more than 1024 tokens per sequence");
  return PLIPMI_OK;
}

// The facts of a model that follow from its validated config alone (the weight pointers come from carve_weights)
inline void init_model(Model* m, const plipmi_config& g) {
  m->cfg = g;
  m->dtype = g.compute_dtype;
  m->esz = m->half() ? 2 : 4;
  m->ln_fold = m->half() && !(g.flags & PLIPMI_FLAG_SEPARATE_LAYERNORM);
  m->pooled_last = m->ln_fold && !(g.flags & PLIPMI_FLAG_DENSE_LAST_BLOCK);
  m->kpad = (int)align_up((size_t)3 * g.patch_size * g.patch_size, 64);
  m->vis.D = g.v_width; m->vis.F = g.v_mlp; m->vis.L = g.v_layers; m->vis.H = g.v_heads;
  m->txt.D = g.t_width; m->txt.F = g.t_mlp; m->txt.L = g.t_layers; m->txt.H = g.t_heads;
  m->vis.dtype = m->dtype;
  m->txt.dtype = (g.flags & PLIPMI_FLAG_TEXT_TOWER_F16) ? PLIPMI_F16 : m->dtype;
  m->txt.lead_f16 = m->txt.dtype == PLIPMI_BF16 ? g.text_f16_layers : 0;
  m->vis.gelu = (g.flags & PLIPMI_FLAG_VISION_GELU) != 0;
  m->txt.gelu = (g.flags & PLIPMI_FLAG_TEXT_GELU) != 0;
}

// plipmi_clone_resolution's argument checks; *max_batch_out = the derived handle's batch (max_batch 0: the largest batch whose
// vision rows fit the source's, B * tokens <= src max_batch * src tokens, at least 1)
inline int check_resolution(const plipmi_engine* src, int height, int width, int max_batch, int* max_batch_out) {
  const int P = src->cfg().patch_size;
  if (height < P || width < P)
    return fail(PLIPMI_ERR_INVALID, "image %d x %d: each side must be at least one patch (%d pixels)", height, width, P);
  const int gh = height / P, gw = width / P;
  const long long tokens = 1 + (long long)gh * gw;
  if (tokens > 1024)
    return fail(PLIPMI_ERR_INVALID, "image %d x %d: a %d x %d grid of %d-pixel patches is %lld tokens, more than 1024 per sequence",
                height, width, gh, gw, P, tokens);
  if (max_batch < 0) return fail(PLIPMI_ERR_INVALID, "max_batch = %d: 0 (derive it from the source's workspace) or positive", max_batch);
  *max_batch_out = max_batch > 0 ? max_batch : (int)std::max(1LL, (long long)src->max_batch * src->vis.S / tokens);
  return PLIPMI_OK;
}

// The vision tower's input geometry: img_h x img_w pixels -> a (img_h / patch) x (img_w / patch) grid, 1 + grid tokens.
inline void set_vision_shape(plipmi_engine* e, int img_h, int img_w) {
  const int P = e->cfg().patch_size;
  e->img_h = img_h; e->img_w = img_w;
  e->gh = img_h / P; e->gw = img_w / P;
  e->np = e->gh * e->gw;
  e->vis.S = e->np + 1;
}

// Per-handle decisions that follow from the handle's max_batch and the token counts (plipmi_create, and plipmi_clone_resolution at
// its own vision token count): pass_batch, the small-batch graph shapes, the attention kernels.  (Whether the fused q/k/v + attention
// kernel and the im2col-on-load patch GEMM apply is decided per call from the tower's S and the batch.)
inline void resolve_handle(plipmi_engine* e) {
  const plipmi_config& g = e->cfg();
  {
    // per-sample bytes of one block's activations in the larger tower: q/k/v (3D) + attention output (D) + the two residual planes
    // (2D) + the MLP hidden (F), 16-bit each (the fp32 engine: twice that and no planes -- the same rule errs on the safe side)
    auto per_sample = [&](int S, int D, int F) { return (double)S * (3.0 * D + D + 2.0 * D + F) * (double)(g.compute_dtype == PLIPMI_F32 ? 4 : 2); };
    const double ps = std::max(per_sample(e->vis.S, g.v_width, g.v_mlp), per_sample(g.context_length, g.t_width, g.t_mlp));
    const int fit = (int)(208e6 / ps) / 32 * 32;       // 208 MB: the cache minus a tower's block weights and the other tower's share
    // passes under 256 samples cost more in the GEMMs (tile quantisation, the 128x128 tile below 12 800 rows) than the cache returns:
    // the fp32 ViT-B/32 engine (fit = 128) ran bs = 256 as two passes at 10.1 k img/s instead of one at 12.5 k
    e->pass_batch = g.pass_batch > 0 ? g.pass_batch : (g.pass_batch == 0 && fit >= 256) ? fit : 0;
  }
  e->graph_batch_cap = std::min(e->max_batch, 32);
  e->graph_batch = g.graph_batch < 0 ? 0 : g.graph_batch == 0 ? e->graph_batch_cap : std::min(g.graph_batch, e->graph_batch_cap);
  // attention kernel: exact-fp32 VALU kernel for the fp32 engine, MFMA kernels for the 16-bit engines
  // (PLIPMI_FLAG_VALU_ATTENTION forces the VALU kernel for A/B runs)
  e->attn_impl = (g.flags & PLIPMI_FLAG_VALU_ATTENTION) ? 0 : PLIPMI_DEFAULT_ATTENTION;
  if (!e->half()) e->attn_impl = 0;
  e->attn_impl_txt = e->attn_impl ? 1 : 0;  // S <= 128: single-pass MFMA kernel, longer: chunked online softmax
  e->attn_impl_vis = e->attn_impl ? 1 : 0;
}

// A handle's shape and settings at max_batch samples of img_h x img_w images: everything a constructor path decides before it
// allocates (plipmi_create: the model's own image size; plipmi_clone / plipmi_clone_resolution: then the source's setter state)
inline void shape_handle(plipmi_engine* e, int max_batch, int img_h, int img_w) {
  e->max_batch = max_batch;
  set_vision_shape(e, img_h, img_w);
  resolve_handle(e);
  e->text_pack = e->model->pooled_last && (e->cfg().flags & PLIPMI_FLAG_PACK_CAPTIONS);
  e->latency_batch = e->half() ? kLatencyBatch : 0;
}

// plipmi_config.pass_batch: how many equal passes an encode call of B samples runs as (1 = the whole batch at once), and the
// rows of pass i -- the first B % n passes take one sample more
inline int passes_of(int pass_batch, int B) { return (pass_batch > 0 && B >= 2 * pass_batch) ? (B + pass_batch - 1) / pass_batch : 1; }
inline int pass_rows(int B, int n, int i) { return B / n + (i < B % n ? 1 : 0); }

// The model's slab: the packed weights (plipmi_create; clones share the model).  CarverT: handle.h Carver (a test's may record the regions)
template <typename CarverT>
void carve_weights(Model* m, CarverT& c) {
  const plipmi_config& g = m->cfg;
  const size_t es = m->esz;
  m->patch_w = c.template take<void>((size_t)g.v_width * m->kpad, es);
  m->cls = c.template take<float>(g.v_width, 4);
  m->vpos_native = c.template take<float>((size_t)m->native_tokens() * g.v_width, 4);
  m->pre_w = c.template take<float>(g.v_width, 4);  m->pre_b = c.template take<float>(g.v_width, 4);
  m->vis.head_ln_w = c.template take<float>(g.v_width, 4); m->vis.head_ln_b = c.template take<float>(g.v_width, 4);
  m->vis.proj_t = c.template take<float>((size_t)g.v_width * g.projection_dim, 4);
  m->tok = c.template take<float>((size_t)g.vocab_size * g.t_width, 4);
  m->tpos = c.template take<float>((size_t)g.context_length * g.t_width, 4);
  m->txt.head_ln_w = c.template take<float>(g.t_width, 4);  m->txt.head_ln_b = c.template take<float>(g.t_width, 4);
  m->txt.proj_t = c.template take<float>((size_t)g.t_width * g.projection_dim, 4);
  m->vis.proj = c.template take<float>((size_t)g.v_width * g.projection_dim, 4);
  m->txt.proj = c.template take<float>((size_t)g.t_width * g.projection_dim, 4);
  for (TowerModel* t : {&m->vis, &m->txt}) {
    const size_t D = t->D, F = t->F;
    t->layers.resize(t->L);
    for (LayerW& w : t->layers) {
      w.wo = c.template take<void>(D * D, es); w.w2 = c.template take<void>(D * F, es);
      w.wqkv = c.template take<void>(3 * D * D, es); w.w1 = c.template take<void>(F * D, es);
      w.bqkv = c.template take<float>(3 * D, 4); w.bo = c.template take<float>(D, 4); w.b1 = c.template take<float>(F, 4); w.b2 = c.template take<float>(D, 4);
      w.ln1w = c.template take<float>(D, 4); w.ln1b = c.template take<float>(D, 4); w.ln2w = c.template take<float>(D, 4); w.ln2b = c.template take<float>(D, 4);
    }
  }
}

// A handle's slab: the workspace of both towers for max_batch samples, the patch rows and the graph staging buffers
template <typename CarverT>
void carve_workspace(plipmi_engine* e, CarverT& c) {
  const Model& m = *e->model;
  const plipmi_config& g = m.cfg;
  const size_t es = m.esz;
  const size_t B = (size_t)e->max_batch;
  e->vis.pooled = c.template take<float>(B * g.v_width, 4);
  e->txt.pooled = c.template take<float>(B * g.t_width, 4);
  for (Tower* t : {&e->vis, &e->txt}) {
    const size_t D = t->m->D, F = t->m->F;
    const size_t M = B * t->S;
    t->x = c.template take<float>(M * D, 4);
    t->h = c.template take<void>(M * D, es);
    if (m.ln_fold) { t->st = c.template take<float>(M * (D / kLnSlice) * 2, 4); t->lo = c.template take<void>(lo_plane_bytes(M, D), 1); }
    if (m.ln_fold && t == &e->txt) {
      t->cu = c.template take<int>(B + 1, 4); t->rowmap = c.template take<int>(M, 4); t->mdev = c.template take<int>(1, 4);
    }
    if (m.pooled_last) {
      t->xp = c.template take<float>(B * D, 4); t->attp = c.template take<void>(B * D, es); t->hp = c.template take<void>(B * D, es);
      t->mlpp = c.template take<void>(B * F, es); t->stp = c.template take<float>(B * (D / kLnSlice) * 2, 4);
    }
    t->qkv = c.template take<void>(M * 3 * D, es);
    t->att = c.template take<void>(M * D, es);
    t->mlp = c.template take<void>(M * F, es);
  }
  e->patches = c.template take<void>(B * e->np * m.kpad, es);
  const size_t gb = (size_t)e->graph_batch_cap;
  if (gb) {
    e->g_vin = c.template take<void>(gb * 3 * e->img_h * e->img_w, 4);
    e->g_tin = c.template take<int64_t>(gb * g.context_length, 8);
    e->g_tmask = c.template take<int64_t>(gb * g.context_length, 8);
    e->g_vout = c.template take<float>(gb * g.projection_dim, 4);
    e->g_tout = c.template take<float>(gb * g.projection_dim, 4);
  }
}

}  // namespace plipmi
