// engine.hip -- the life of a handle (include/plipmi.h): create, clone, destroy, the per-handle setters and the event-based
// per-kernel profile.  The towers' drivers and encode entries are in towers.hip, the heads (logits, top-k, resize, linear probe)
// in heads.hip, the kernel-level test entries in test_entries.hip; the types they share are in handle.h / handle_host.h.
//
// Data layout in HBM
//   weights    one slab per MODEL, shared by a handle and its clones (handle.h Model): per layer Wqkv [3D,D] (q rows pre-scaled by
//              head^-1/2: 1/8 at head 64, exact), Wo [D,D], W1 [F,D], W2 [D,F] in the tower's operand type, K contiguous (= the HF [out,in]
//              layout, so no transposes) -- on a LayerNorm-folded engine Wqkv / W1 carry the LayerNorm gain and centring;
//              biases / LayerNorm / embeddings fp32; projection matrices fp32 as [P,D] and transposed [D,P].
//   workspace  one slab per HANDLE, sized for its max_batch (handle.h Tower; M = B * tokens): per tower x fp32 [M,D] (embedding
//              rows, joined copies), qkv [M,3D], att [M,D], mlp [M,F] in the operand type; 16-bit engines keep the residual stream
//              as two planes -- h [M,D] operand type + lo 8-bit remainder -- with the rows' LayerNorm statistics st [M,D/64,2];
//              the pooled last block's [B,*] rows; the patch rows; the staging buffers of the captured small-batch graphs.
//              The two towers have separate workspaces so they can run on two streams.
#include <math.h>
#include <stdio.h>
#include <time.h>

#include "handle_host.h"

namespace plipmi {

thread_local char g_err[512] = "";
int g_fuse_qkv_attention = 1;
int g_patch_gather = 1;
unsigned g_hook_epoch = 0;

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// a token id outside the vocabulary seen by an EARLIER encode_text (the flag is written by the device, so it is known only
// once that work has run): report once, then clear
int check_async(plipmi_engine* e) {
  if (e->bad_id && *reinterpret_cast<volatile int*>(e->bad_id) != 0) {
    *reinterpret_cast<volatile int*>(e->bad_id) = 0;
    return fail(PLIPMI_ERR_TOKEN_ID, "an earlier plipmi_encode_text on this handle was given a token id outside [0, %d) "
                "(the reference's embedding lookup raises there, plip.py:68); its embeddings are invalid", e->cfg().vocab_size);
  }
  return PLIPMI_OK;
}
// (the sticky token-id flag is reported by plipmi_encode_text and plipmi_check_async only: a bad caption must not fail an
//  unrelated encode_image, and whether it did used to depend on whether the embedding kernel had already run)
int check_batch(plipmi_engine* e, int B) {
  if (!e) return fail(PLIPMI_ERR_INVALID, "null handle");
  if (B < 0 || B > e->max_batch)
    return fail(PLIPMI_ERR_INVALID, "batch %d outside [0, max_batch=%d]", B, e->max_batch);
  return PLIPMI_OK;
}

}  // namespace plipmi

using namespace plipmi;

namespace {

int pack_tower(const Model& m, const TowerModel& t, const plipmi_layer_weights* src, hipStream_t s) {
  const int D = t.D, F = t.F;
  // head_dim^-0.5 folded into Wq / bq: computed in double and rounded once to fp32.  Head 64: exactly 0.125, a power of two, so
  // the fold is exact; any other head (72 .. 128) rounds the scaled weights once more, in fp32, before their operand rounding
  const float qscale = (float)(1.0 / sqrt((double)t.head()));
  for (int l = 0; l < t.L; ++l) {
    const int dt = t.layer_dtype(l);
    const plipmi_layer_weights& w = src[l];
    const LayerW& d = t.layers[l];
    char* wq = reinterpret_cast<char*>(d.wqkv);
    if (m.ln_fold) {
      // W' = (W * g, rows centred) in the operand type (q rows also x 1/8), c2 = W b_ln + bias -> the bias slot
      HIP_TRY(launch_fold_ln(w.q_w, w.q_b, w.ln1_w, w.ln1_b, wq, d.bqkv, D, D, qscale, dt, s));
      HIP_TRY(launch_fold_ln(w.k_w, w.k_b, w.ln1_w, w.ln1_b, wq + (size_t)D * D * m.esz, d.bqkv + D, D, D, 1.f, dt, s));
      HIP_TRY(launch_fold_ln(w.v_w, w.v_b, w.ln1_w, w.ln1_b, wq + (size_t)2 * D * D * m.esz, d.bqkv + 2 * D, D, D, 1.f, dt, s));
      HIP_TRY(launch_fold_ln(w.fc1_w, w.fc1_b, w.ln2_w, w.ln2_b, d.w1, d.b1, F, D, 1.f, dt, s));
    } else {
      HIP_TRY(launch_convert(w.q_w, wq, dt, D, D, D, qscale, s));
      HIP_TRY(launch_convert(w.k_w, wq + (size_t)D * D * m.esz, dt, D, D, D, 1.f, s));
      HIP_TRY(launch_convert(w.v_w, wq + (size_t)2 * D * D * m.esz, dt, D, D, D, 1.f, s));
      HIP_TRY(launch_convert(w.fc1_w, d.w1, dt, F, D, D, 1.f, s));
      HIP_TRY(launch_scale_copy(w.q_b, d.bqkv, D, qscale, s));
      HIP_TRY(launch_scale_copy(w.k_b, d.bqkv + D, D, 1.f, s));
      HIP_TRY(launch_scale_copy(w.v_b, d.bqkv + 2 * D, D, 1.f, s));
      HIP_TRY(launch_scale_copy(w.fc1_b, d.b1, F, 1.f, s));
    }
    HIP_TRY(launch_convert(w.o_w, d.wo, dt, D, D, D, 1.f, s));
    HIP_TRY(launch_convert(w.fc2_w, d.w2, dt, D, F, F, 1.f, s));
    HIP_TRY(launch_scale_copy(w.o_b, d.bo, D, 1.f, s));
    HIP_TRY(launch_scale_copy(w.fc2_b, d.b2, D, 1.f, s));
    HIP_TRY(launch_scale_copy(w.ln1_w, d.ln1w, D, 1.f, s));
    HIP_TRY(launch_scale_copy(w.ln1_b, d.ln1b, D, 1.f, s));
    HIP_TRY(launch_scale_copy(w.ln2_w, d.ln2w, D, 1.f, s));
    HIP_TRY(launch_scale_copy(w.ln2_b, d.ln2b, D, 1.f, s));
  }
  return PLIPMI_OK;
}

// the checkpoint's tensors into the model's slab, in the layouts the kernels read
int pack_model(const Model& m, const plipmi_weights* w, hipStream_t s) {
  const plipmi_config& g = m.cfg;
  const int Dv = g.v_width, Dt = g.t_width, P = g.projection_dim;
  HIP_TRY(launch_convert(w->v_patch_weight, m.patch_w, m.vis.dtype, Dv, 3 * g.patch_size * g.patch_size, m.kpad, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_class_embedding, m.cls, Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_pos_embedding, m.vpos_native, m.native_tokens() * Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_pre_ln_w, m.pre_w, Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_pre_ln_b, m.pre_b, Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_post_ln_w, m.vis.head_ln_w, Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->v_post_ln_b, m.vis.head_ln_b, Dv, 1.f, s));
  HIP_TRY(launch_transpose(w->visual_projection, m.vis.proj_t, P, Dv, s));
  HIP_TRY(launch_scale_copy(w->visual_projection, m.vis.proj, P * Dv, 1.f, s));
  HIP_TRY(launch_scale_copy(w->text_projection, m.txt.proj, P * Dt, 1.f, s));
  HIP_TRY(hipMemcpyAsync(m.tok, w->t_token_embedding, (size_t)g.vocab_size * Dt * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(launch_scale_copy(w->t_pos_embedding, m.tpos, g.context_length * Dt, 1.f, s));
  HIP_TRY(launch_scale_copy(w->t_final_ln_w, m.txt.head_ln_w, Dt, 1.f, s));
  HIP_TRY(launch_scale_copy(w->t_final_ln_b, m.txt.head_ln_b, Dt, 1.f, s));
  HIP_TRY(launch_transpose(w->text_projection, m.txt.proj_t, P, Dt, s));
  RUN(pack_tower(m, m.vis, w->v_layers, s));
  RUN(pack_tower(m, m.txt, w->t_layers, s));
  return PLIPMI_OK;
}

// hipMalloc the handle's workspace slab and hand out its pointers
int alloc_workspace(plipmi_engine* e) {
  Carver sizing;
  carve_workspace(e, sizing);
  RUN(e->slab.reserve(align_up(sizing.off, 256), nullptr));
  Carver placing;
  placing.base = e->slab.data();
  carve_workspace(e, placing);
  if (e->bad_id_mem.reserve(sizeof(int), nullptr) == PLIPMI_OK) {   // (no flag memory: out-of-range ids go unreported)
    e->bad_id = reinterpret_cast<int*>(e->bad_id_mem.data());
    *e->bad_id = 0;
  }
  return PLIPMI_OK;
}

// A handle on src's model at max_batch samples of height x width images, with src's setter state and a workspace of its own
int derive(plipmi_handle src, int max_batch, int height, int width, std::unique_ptr<plipmi_engine>* out) {
  auto e = std::make_unique<plipmi_engine>(src->model);
  shape_handle(e.get(), max_batch, height, width);
  e->graph_batch = std::min(src->graph_batch, e->graph_batch_cap);   // the source's setter state, within this handle's staging
  e->latency_batch = src->latency_batch;
  e->text_pack = src->text_pack;
  e->vpos = src->model->vpos_native;
  RUN(alloc_workspace(e.get()));
  *out = std::move(e);
  return PLIPMI_OK;
}

}  // namespace

extern "C" {

int plipmi_version(void) { return PLIPMI_VERSION; }
const char* plipmi_last_error(void) { return g_err; }
const char* plipmi_device_name(plipmi_handle h) { return h ? h->model->devname : ""; }

int plipmi_create(const plipmi_config* cfg, const plipmi_weights* w, void* stream, plipmi_handle* out) {
  if (!cfg || !w || !out) return fail(PLIPMI_ERR_INVALID, "null argument");
  *out = nullptr;
  plipmi_config g;
  RUN(validate_config(cfg, &g));

  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
    return fail(PLIPMI_ERR_NODEVICE, "no HIP device visible (libplipmi needs an MI355X / gfx950 GPU)");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(PLIPMI_ERR_NODEVICE, "device %d is %s; libplipmi is built for gfx950 only", dev, prop.gcnArchName);

  auto m = std::make_shared<Model>();
  init_model(m.get(), g);
  snprintf(m->devname, sizeof(m->devname), "%s:%s", prop.gcnArchName, prop.name);
  Carver sizing;
  carve_weights(m.get(), sizing);
  RUN(m->slab.reserve(align_up(sizing.off, 256), nullptr));
  Carver placing;
  placing.base = m->slab.data();
  carve_weights(m.get(), placing);

  auto e = std::make_unique<plipmi_engine>(m);
  shape_handle(e.get(), g.max_batch, g.image_size, g.image_size);
  e->vpos = m->vpos_native;
  RUN(alloc_workspace(e.get()));
  RUN(pack_model(*m, w, reinterpret_cast<hipStream_t>(stream)));
  *out = e.release();
  return PLIPMI_OK;
}

int plipmi_clone(plipmi_handle src, plipmi_handle* out) {
  if (!src || !out) return fail(PLIPMI_ERR_INVALID, "null argument");
  *out = nullptr;
  std::unique_ptr<plipmi_engine> e;
  RUN(derive(src, src->max_batch, src->img_h, src->img_w, &e));
  e->vpos = src->vpos;             // src's image size, hence its position table (a resampled one is shared)
  e->vpos_own = src->vpos_own;
  *out = e.release();
  return PLIPMI_OK;
}

int plipmi_clone_resolution(plipmi_handle src, int height, int width, int max_batch, plipmi_handle* out) {
  if (!src || !out) return fail(PLIPMI_ERR_INVALID, "null argument");
  *out = nullptr;
  int B = 0;
  RUN(check_resolution(src, height, width, max_batch, &B));
  std::unique_ptr<plipmi_engine> e;
  RUN(derive(src, B, height, width, &e));
  // HF interpolate_pos_encoding: the checkpoint's table as it is for its own patch count on a square image, else CLS + the bicubic
  // resample of the n0 x n0 patch rows to gh x gw -- computed once, here
  const plipmi_config& g = src->cfg();
  const int n0 = g.image_size / g.patch_size;
  if (!(e->np == n0 * n0 && height == width)) {
    e->vpos_own = std::make_shared<Buffer>();
    RUN(e->vpos_own->reserve((size_t)e->vis.S * g.v_width * 4, nullptr));
    e->vpos = reinterpret_cast<float*>(e->vpos_own->data());
    // the legacy stream orders after the weights' packing on any blocking stream; synchronised: the table is ready for every stream
    hipError_t le = launch_resample_pos(e->model->vpos_native, e->vpos, n0, e->gh, e->gw, g.v_width, nullptr);
    if (le == hipSuccess) le = hipStreamSynchronize(nullptr);
    if (le != hipSuccess)
      return fail(PLIPMI_ERR_HIP, "position table resample (%d x %d -> %d x %d) failed: %s", n0, n0, e->gh, e->gw, hipGetErrorString(le));
  }
  *out = e.release();
  return PLIPMI_OK;
}

void plipmi_destroy(plipmi_handle h) { delete h; }

int plipmi_check_async(plipmi_handle h) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "null handle");
  return check_async(h);
}

int plipmi_set_graph_batch(plipmi_handle h, int max_batch) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "null handle");
  h->graph_batch = std::max(0, std::min(max_batch, h->graph_batch_cap));
  return PLIPMI_OK;
}

int plipmi_get_pass_batch(plipmi_handle h) { return h ? h->pass_batch : 0; }

int plipmi_set_latency_batch(plipmi_handle h, int max_batch) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "null handle");
  const int v = h->half() ? std::max(0, max_batch) : 0;
  if (v != h->latency_batch) h->graphs.clear();       // captured forwards hold the other regime's launches
  h->latency_batch = v;
  return PLIPMI_OK;
}

int plipmi_set_text_packing(plipmi_handle h, int on) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "null handle");
  if (on && !h->model->pooled_last)
    return fail(PLIPMI_ERR_INVALID, "caption packing needs a 16-bit engine's pooled last block (compute_dtype bf16 / f16, LayerNorm folding on, last block not dense)");
  if (on && h->model->txt.head() != 64)
    return fail(PLIPMI_ERR_INVALID, "caption packing needs a text tower with head_dim 64: packed rows are a form of the head-64 short-sequence "
                "attention kernel (this tower: t_width=%d/%d heads = %d)", h->model->txt.D, h->model->txt.H, h->model->txt.head());
  if ((on != 0) != h->text_pack) h->graphs.clear();   // captured text forwards hold the other form's launches
  h->text_pack = on != 0;
  return PLIPMI_OK;
}

int plipmi_tower_shape(plipmi_handle h, int tower, int32_t* shape) {
  if (!h || !shape) return fail(PLIPMI_ERR_INVALID, "null handle/shape");
  if (!valid_tower(tower)) return fail(PLIPMI_ERR_INVALID, "tower must be 0 (vision) or 1 (text), got %d", tower);
  const Tower& t = tower == PLIPMI_VISION ? h->vis : h->txt;
  shape[0] = t.S; shape[1] = t.m->D; shape[2] = t.m->H; shape[3] = t.m->L;
  return PLIPMI_OK;
}

int plipmi_streams_overlap(plipmi_handle h, void* stream_a, void* stream_b, float* ratio) {
  if (!h || !ratio) return fail(PLIPMI_ERR_INVALID, "bad argument");
  hipStream_t sa = reinterpret_cast<hipStream_t>(stream_a), sb = reinterpret_cast<hipStream_t>(stream_b);
  int dev = 0, khz = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
  const double us = 250.0;
  const unsigned long long ticks = (unsigned long long)(us * 1e-3 * khz);
  HIP_TRY(launch_occupy(ticks / 8, sa));            // code object loaded, queues awake
  HIP_TRY(launch_occupy(ticks / 8, sb));
  double best = 1e30;
  for (int rep = 0; rep < 3; ++rep) {               // the shortest of three: a host hiccup only ever lengthens a window
    HIP_TRY(hipStreamSynchronize(sa));
    HIP_TRY(hipStreamSynchronize(sb));
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    HIP_TRY(launch_occupy(ticks, sa));
    HIP_TRY(launch_occupy(ticks, sb));
    HIP_TRY(hipStreamSynchronize(sa));
    HIP_TRY(hipStreamSynchronize(sb));
    clock_gettime(CLOCK_MONOTONIC, &t1);
    best = std::min(best, (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3);
  }
  *ratio = (float)(best / us);
  return PLIPMI_OK;
}

int plipmi_profile_enable(plipmi_handle h, int on) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "null handle");
  Profile& p = h->prof;
  if (on) {
    for (ProfRec& r : p.recs) { p.pool.push_back(r.t0); p.pool.push_back(r.t1); }
    p.recs.clear();
  }
  p.on = on != 0;
  return PLIPMI_OK;
}

int plipmi_profile_read(plipmi_handle h, plipmi_kernel_stat* rows, int max_rows, int* n_rows) {
  if (!h || !rows || !n_rows || max_rows <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  HIP_TRY(hipDeviceSynchronize());
  int n = 0;
  for (ProfRec& r : h->prof.recs) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.t0, r.t1));
    int k = 0;
    for (; k < n; ++k)
      if (strncmp(rows[k].name, r.name, sizeof(rows[k].name) - 1) == 0) break;
    if (k == n) {
      if (n == max_rows) continue;
      memset(&rows[n], 0, sizeof(rows[n]));
      strncpy(rows[n].name, r.name, sizeof(rows[n].name) - 1);
      ++n;
    }
    rows[k].calls += 1;
    rows[k].total_ms += ms;
    rows[k].flops += r.flops;
    rows[k].bytes += r.bytes;
  }
  *n_rows = n;
  return PLIPMI_OK;
}

}  // extern "C"
