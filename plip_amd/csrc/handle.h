// handle.h -- what a plipmi handle is made of, shared by the host translation units of libplipmi.so (engine.hip, towers.hip,
// heads.hip, test_entries.hip): the error slot, the owning resource types, the model a handle and its clones share, the state
// every handle builds for itself, and the per-call forward context.
//
// Ownership in one paragraph: a `Model` (validated config, packed weights and the slab that holds them) is immutable and shared
// through one shared_ptr by a handle and every handle derived from it.  Everything else a `plipmi_engine` holds -- workspace slab,
// captured graphs, scratch buffers, profile events -- belongs to that handle alone and sits in move-only owning types, so a handle
// cannot be copied (static_assert below) and `delete h` releases exactly what h allocated, whatever order handles are destroyed in.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/plipmi.h"
#include "../../include/plipmi_test.h"
#include "gemm.h"
#include "kernels.h"

namespace plipmi {

// ---- process-wide state: one definition each, in engine.hip -----------------------------------------------------------------
extern thread_local char g_err[512];
// TEST / A-B hooks (plipmi_test.h, process-wide; the product path never writes them).
// g_fuse_qkv_attention (plipmi_test_fused_qkv_attention): 0 = the text tower's q/k/v projection and its attention run as two kernels
// even where the fused kernel (qkv_attention.hip) applies, 1 = the product rule (fused where it applies AND the batch fills the chip),
// 2 = fused wherever it applies, small batches too.
extern int g_fuse_qkv_attention;
// g_patch_gather (plipmi_test_patch_gather): 0 = pixels always go through the unfold pass + the plain patch GEMM, 1 (default) = the
// patch GEMM gathers them itself where gemm_gather_supports() says so.
extern int g_patch_gather;
// Captured hipGraphs hold the launches of the hook settings they were captured under: every hook change bumps this epoch, and a handle
// whose graphs are older drops them before its next small-batch call.
extern unsigned g_hook_epoch;

int fail(int code, const char* fmt, ...);   // writes the thread's plipmi_last_error text, returns code

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(PLIPMI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define RUN(expr) do { int rc_ = (expr); if (rc_ != PLIPMI_OK) return rc_; } while (0)

inline bool half_code(int dtype) { return dtype == PLIPMI_BF16 || dtype == PLIPMI_F16; }
inline bool valid_dtype(int dtype) { return dtype == PLIPMI_F32 || half_code(dtype); }
inline bool valid_tower(int tower) { return tower == PLIPMI_VISION || tower == PLIPMI_TEXT; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What every head on cached embeddings asks of X [N, D] fp32 (heads.hip probe_check / softmax_check, kmeans.hip km_check): rows, a width
// probe_tile.h has a tile for, 16-byte loads.  `who` ("" or "entry: ") goes in front of the message.
inline int check_embeddings(const char* who, const void* X, int N, int D) {
  if (N <= 0) return fail(PLIPMI_ERR_INVALID, "%sneed N > 0 rows, got %d", who, N);
  if (D < 4 || D > 1024 || D % 4) return fail(PLIPMI_ERR_INVALID, "%sembedding width %d unsupported (D %% 4 == 0, 4 <= D <= 1024)", who, D);
  if (reinterpret_cast<uintptr_t>(X) % 16) return fail(PLIPMI_ERR_INVALID, "%sX must be 16-byte aligned", who);
  return PLIPMI_OK;
}

struct Carver {  // two-pass slab carving: pass 1 sizes (base == nullptr), pass 2 hands out pointers
  char* base = nullptr;
  size_t off = 0;
  template <typename T> T* take(size_t count, size_t elem) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * elem;
    return p;
  }
};

// ---- owning resource types (move-only or pinned in place: never copied) -----------------------------------------------------
// One allocation, grown on demand: device memory or pinned host memory.  reserve() keeps the buffer when it is large enough;
// otherwise it waits for the stream that may still be using the old one, frees it and allocates the request.
class Buffer {
 public:
  enum Kind { kDevice, kPinned, kPinnedMapped };
  explicit Buffer(Kind kind = kDevice) : kind_(kind) {}
  Buffer(Buffer&& o) noexcept : kind_(o.kind_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { release(); kind_ = o.kind_; p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~Buffer() { release(); }
  int reserve(size_t bytes, hipStream_t s) {
    if (bytes <= cap_) return PLIPMI_OK;
    if (p_) { HIP_TRY(hipStreamSynchronize(s)); release(); }
    const hipError_t me = kind_ == kDevice ? hipMalloc(reinterpret_cast<void**>(&p_), bytes)
                                           : hipHostMalloc(reinterpret_cast<void**>(&p_), bytes,
                                                           kind_ == kPinned ? hipHostMallocDefault : hipHostMallocMapped);
    if (me != hipSuccess) {
      p_ = nullptr;
      return fail(PLIPMI_ERR_NOMEM, "%s(%zu bytes) failed: %s", kind_ == kDevice ? "hipMalloc" : "hipHostMalloc", bytes, hipGetErrorString(me));
    }
    cap_ = bytes;
    return PLIPMI_OK;
  }
  char* data() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  void release() {
    if (p_) { if (kind_ == kDevice) hipFree(p_); else hipHostFree(p_); }
    p_ = nullptr; cap_ = 0;
  }
  Kind kind_;
  char* p_ = nullptr;
  size_t cap_ = 0;
};

// One captured tower forward (hipGraph) per (input kind, batch, normalise, eos id, mask?): the ~170 launches of a small-batch
// encode are replayed with ONE host call instead of being issued one by one (launch-bound at the reference's own batch size
// of 8, plip.py:90-91).  Inputs / outputs of a captured forward live in handle-owned staging buffers, because the caller's
// pointers change from call to call and graph nodes hold theirs fixed.
struct GraphEntry {
  int seen = 0;                 // calls so far: the first runs eagerly (it also sets the kernels' attributes)
  hipGraphExec_t exec = nullptr;
};
class GraphCache {
 public:
  using Key = std::tuple<int, int, int, int, int>;
  GraphCache() = default;
  GraphCache(const GraphCache&) = delete;
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() {
    clear();
    if (stream_) hipStreamDestroy(stream_);
  }
  void clear() {                // captured forwards hold the launches of the settings they were captured under
    for (auto& kv : entries_) if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
    entries_.clear();
  }
  GraphEntry& at(const Key& k) {
    if (epoch_ != g_hook_epoch) {   // a test hook changed what the launches are since these graphs were captured
      clear();
      epoch_ = g_hook_epoch;
    }
    return entries_[k];
  }
  // captures run here: the legacy default stream cannot capture, and the caller's stream never enters capture mode (other threads
  // may be enqueueing on it)
  hipError_t capture_stream(hipStream_t* out) {
    const hipError_t e = stream_ ? hipSuccess : hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
    *out = stream_;
    return e;
  }

 private:
  std::map<Key, GraphEntry> entries_;
  unsigned epoch_ = 0;          // g_hook_epoch the captured graphs belong to
  hipStream_t stream_ = nullptr;
};

struct ProfRec {
  const char* name;
  hipEvent_t t0, t1;
  double flops, bytes;
};
struct Profile {                // event-based per-kernel profile (plipmi_profile_enable / _read)
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  Profile() = default;
  Profile(const Profile&) = delete;
  Profile& operator=(const Profile&) = delete;
  ~Profile() {
    for (ProfRec& r : recs) { hipEventDestroy(r.t0); hipEventDestroy(r.t1); }
    for (hipEvent_t ev : pool) hipEventDestroy(ev);
  }
};

// ---- the model: immutable, shared by a handle and every handle cloned or derived from it -----------------------------------
struct LayerW {
  void *wqkv, *wo, *w1, *w2;
  float *bqkv, *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
  // LayerNorm-folded engine: wqkv / w1 hold the centred W * g (LayerNorm gain and mean subtraction folded in),
  // bqkv / b1 hold c2 = W b_ln + bias
};
struct TowerModel {
  int D = 0, F = 0, L = 0, H = 0;
  int head() const { return D / H; }   // columns of one attention head: 64, or 72 .. 128 in steps of 8 (validate_config)
  int dtype = 0;   // operand type of this tower's GEMMs / attention (the engine's, or f16 for the text tower under PLIPMI_FLAG_TEXT_TOWER_F16)
  // plipmi_config.text_f16_layers: the first lead_f16 blocks of a bf16 text tower run on IEEE-half operands (the blocks where
  // bf16's operand rounding costs the embeddings most -- DESIGN.md section 2.1), the rest on the tower's type.
  int lead_f16 = 0;
  int layer_dtype(int l) const { return l < lead_f16 ? PLIPMI_F16 : dtype; }
  // MLP activation of this tower's blocks: QuickGELU (HF hidden_act "quick_gelu"), or the exact erf GELU ("gelu";
  // PLIPMI_FLAG_VISION_GELU / PLIPMI_FLAG_TEXT_GELU) -- the fc1 GEMM's epilogue kind, plain and LayerNorm-folded
  bool gelu = false;
  int fc1_epi(bool ln_folded) const { return ln_folded ? (gelu ? EPI_GELU_LN : EPI_QGELU_LN) : (gelu ? EPI_BIAS_GELU : EPI_BIAS_QGELU); }
  std::vector<LayerW> layers;
  // head of the tower: the LayerNorm in front of the projection, the projection [P, D] fp32 (the HF layout, NT GEMM operand)
  // and its transpose [D, P] (the fused pool_head kernel's)
  float *head_ln_w = nullptr, *head_ln_b = nullptr, *proj = nullptr, *proj_t = nullptr;
};
struct Model {
  plipmi_config cfg;            // as validated by plipmi_create (max_batch: the creating handle's; every handle keeps its own)
  int dtype = 0;
  size_t esz = 4;
  // 16-bit engines: the 2 x L LayerNorms of the blocks are folded into the GEMMs around them (no LayerNorm pass, no
  // normalised activations in memory); PLIPMI_FLAG_SEPARATE_LAYERNORM restores the separate LayerNorm kernels for A/B runs
  bool ln_fold = false;
  // The last block's out_proj / fc1 / fc2 (and both of its residual adds) only ever reach the output through the row that
  // is pooled afterwards (CLS / EOS): the encode paths run them on that one row per sample (PLIPMI_FLAG_DENSE_LAST_BLOCK
  // computes all rows, as plipmi_debug_hidden always does).  LayerNorm-folded engines only.
  bool pooled_last = false;
  int kpad = 0;                 // 3 * patch^2 padded to the GEMM's K tile
  TowerModel vis, txt;          // vis head: post_layernorm + visual_projection; txt head: final_layer_norm + text_projection
  void* patch_w = nullptr;      // [Dv, kpad]
  float *cls = nullptr, *vpos_native = nullptr /* the checkpoint's own n0 x n0 grid */, *pre_w = nullptr, *pre_b = nullptr;
  float *tok = nullptr, *tpos = nullptr;
  Buffer slab;                  // the packed weights: every pointer above points into it
  char devname[128] = "";
  bool half() const { return dtype != PLIPMI_F32; }
  int native_tokens() const { return (cfg.image_size / cfg.patch_size) * (cfg.image_size / cfg.patch_size) + 1; }
};

// ---- per-handle state ----------------------------------------------------------------------------------------------------
struct Tower {                  // one tower's workspace, sized for the handle's max_batch samples of S tokens
  const TowerModel* m = nullptr;
  int S = 0;
  float* x = nullptr;
  void *h = nullptr, *qkv = nullptr, *att = nullptr, *mlp = nullptr;
  // LayerNorm-folded engine: the residual stream lives as two planes (common.h split_f32): h = its operand-type plane
  // (the A operand of the q/k/v and fc1 GEMMs), lo = the 8-bit remainder plane (blocked layout); x only holds the
  // embedding rows before the first LayerNorm and a joined copy where something needs plain fp32.  st = the rows'
  // statistics partials [M, D/64, 2]
  float* st = nullptr;
  void* lo = nullptr;
  // packed captions (text tower, plipmi_set_text_packing): rows past a caption's EOS are not computed; everything about the
  // packing lives on the device -- cu [B+1] row offsets, rowmap [B*S] packed row -> (sample << 8 | position), mdev = live rows
  int *cu = nullptr, *rowmap = nullptr, *mdev = nullptr;
  // last block, pooled rows only (one row per sample): residual row, attention output, bf16 copy, MLP hidden, partials
  float* xp = nullptr; void *attp = nullptr, *hp = nullptr, *mlpp = nullptr; float* stp = nullptr;
  float* pooled = nullptr;      // [max_batch, D] fp32 LayerNorm'd pooled rows (the head GEMM's A operand)
};

}  // namespace plipmi

struct plipmi_engine {
  const std::shared_ptr<const plipmi::Model> model;
  int max_batch = 0;
  // the vision tower's input: img_h x img_w pixels, a gh x gw patch grid (np = gh * gw patches, vis.S = 1 + np tokens).  plipmi_create:
  // the checkpoint's image_size square; plipmi_clone_resolution: any other size, the grid floored like HF's strided conv
  int img_h = 0, img_w = 0, gh = 0, gw = 0, np = 0;
  // vpos = the position table the tower adds ([1 + np, Dv] fp32): the model's own, or -- a handle at another grid -- a resampled
  // table (vpos_own, plipmi_clone_resolution), shared with its plipmi_clone's
  float* vpos = nullptr;
  std::shared_ptr<plipmi::Buffer> vpos_own;
  // ---- settings resolved per handle (handle_host.h resolve_handle) and their setters' state
  // plipmi_config.pass_batch resolved: an encode call of B >= 2 * pass_batch samples runs as equal back-to-back passes of at most
  // pass_batch (0 = never split).  A pass's per-block activations (qkv, att, mlp, the residual planes) then stay in the 256 MiB Infinity
  // Cache whatever the caller's batch: at bs = 512 / 1024 in ONE pass the ViT-B/32 step ran 8 % / 3 % under the bs = 256 rate
  // (BENCH_r05 batch_scaling).  Same bits: a row's embedding does not depend on the batch it travels in.
  int pass_batch = 0;
  // small-batch hipGraph replay (plipmi_config.graph_batch, plipmi_set_graph_batch): batches of at most this many samples;
  // graph_batch_cap = what the staging buffers hold
  int graph_batch = 0, graph_batch_cap = 0;
  // latency path: batches of at most this many samples run their GEMMs on the split-K small-M kernel (16-bit engines).  The
  // reference drives zero_shot_classification / retrieval at batch 8 (plip.py:90-91,112).  Results of the two regimes differ
  // by fp32 summation order only; inside a regime a row's embedding does not depend on the batch it arrives in.
  int latency_batch = 0;
  // Packed captions (plipmi_set_text_packing; PLIPMI_FLAG_PACK_CAPTIONS): the text tower computes rows 0 .. EOS of each caption
  // only -- causal attention and EOS pooling mean the rows behind EOS cannot reach the embedding.  Off by default: the
  // default engine executes every padded position, like the reference does.
  bool text_pack = false;
  int attn_impl = 0, attn_impl_vis = 0, attn_impl_txt = 0;
  // ---- workspace: one slab, carved by handle_host.h carve_workspace
  plipmi::Buffer slab;
  plipmi::Tower vis, txt;
  void* patches = nullptr;      // [max_batch*np, kpad]
  void* g_vin = nullptr;        // staged image input (fp32 pixels or uint8 tiles) [graph_batch_cap, 3, H, W] x 4 B
  int64_t* g_tin = nullptr;     // staged ids   [graph_batch_cap, ctx]
  int64_t* g_tmask = nullptr;   // staged attention mask
  float *g_vout = nullptr, *g_tout = nullptr;   // staged embeddings [graph_batch_cap, P]
  // ---- what the handle allocates as it goes
  plipmi::GraphCache graphs;
  // raised by the embedding kernels when a token id lies outside the vocabulary (host-visible memory; reported by the next
  // call on the handle and by plipmi_check_async -- the reference's lookup raises, plip.py:68)
  plipmi::Buffer bad_id_mem{plipmi::Buffer::kPinnedMapped};
  int* bad_id = nullptr;
  plipmi::Buffer sim_ws;        // plipmi_similarity_topk scratch (allocated on first use, grown on demand)
  // plipmi_encode_attention_summary scratch: the pooled-row indices and the rollout's two [B, S, S] buffers (allocated on first
  // use, grown on demand; never part of the tower workspace)
  plipmi::Buffer summary_ws;
  // plipmi_encode_token_similarity scratch: the post_layernorm'd rows [B*S, Dv] and, when the caller takes no token_embeds, their
  // projections [B*S, P] (allocated on first use, grown on demand; never part of the tower workspace)
  plipmi::Buffer token_ws;
  // linear-probe scratch (plipmi_probe_fit / _predict / _loss_grad): device partials + results, and a pinned host mirror of the
  // trial point, gradient and losses.  Allocations of their own, grown on demand: never part of the tower workspace.
  plipmi::Buffer probe_ws, probe_host{plipmi::Buffer::kPinned};
  // k-means scratch (plipmi_kmeans_seed / _assign / _fit / _update, kmeans.hip): row norms, centre biases, the sorted row order, the
  // per-chunk partial sums and the few bytes a fit reads back; a pinned host mirror for those bytes and for the rare empty-cluster
  // path.  Allocations of their own, grown on demand: never part of the tower workspace.
  plipmi::Buffer kmeans_ws, kmeans_host{plipmi::Buffer::kPinned};
  plipmi::Profile prof;

  explicit plipmi_engine(std::shared_ptr<const plipmi::Model> m) : model(std::move(m)) {
    vis.m = &model->vis;
    txt.m = &model->txt;
    txt.S = model->cfg.context_length;
  }
  const plipmi_config& cfg() const { return model->cfg; }
  bool half() const { return model->half(); }
};
static_assert(!std::is_copy_constructible_v<plipmi_engine> && !std::is_copy_assignable_v<plipmi_engine>,
              "a handle owns its workspace, graphs and scratch: a clone is constructed from the model, never copied");

namespace plipmi {

struct Scope {  // brackets one kernel launch with events while profiling is on
  Profile& p;
  hipStream_t s;
  bool on;
  ProfRec r;
  Scope(plipmi_engine* e, hipStream_t s_, const char* name, double flops, double bytes) : p(e->prof), s(s_), on(e->prof.on) {
    if (!on) return;
    r.name = name; r.flops = flops; r.bytes = bytes;
    r.t0 = take(); r.t1 = take();
    hipEventRecord(r.t0, s);
  }
  void rename(const char* name) { r.name = name; }
  ~Scope() {
    if (!on) return;
    hipEventRecord(r.t1, s);
    p.recs.push_back(r);
  }
  hipEvent_t take() {
    if (!p.pool.empty()) { hipEvent_t ev = p.pool.back(); p.pool.pop_back(); return ev; }
    hipEvent_t ev; hipEventCreate(&ev); return ev;
  }
};

// C[M,N] = A[M,K] . W[N,K]^T with the given leading dimensions; alpha 1, one "patch" per image -- callers set what else they need
inline GemmParams make_params(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda, int ldw, int ldc) {
  GemmParams p;
  p.A = A; p.W = W; p.C = C; p.bias = bias;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc;
  p.alpha = 1.f; p.np = 1;
  return p;
}

int check_batch(plipmi_engine* e, int B);   // engine.hip
int check_async(plipmi_engine* e);

}  // namespace plipmi
