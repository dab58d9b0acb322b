// towers.hip -- the two tower forwards: embeddings, the pre-LN residual blocks, the pooled last block and the projection head,
// and the entries that run them (plipmi_encode_image / _image_u8 / _text, plipmi_encode_tower_outputs, plipmi_debug_hidden).
// A forward is enqueued through a `Forward` context built on the stack by its entry: whatever holds for one call only lives there,
// never on the handle.
#include "handle_host.h"

using namespace plipmi;

namespace {

struct LnArgs {         // the LayerNorm side of a folded GEMM (gemm.h EPI_*_LN / EPI_RESID_EMIT)
  const float* stats = nullptr; int ns = 0; float inv_d = 0.f, eps = 0.f;   // consumer
  void* xb_out = nullptr; float* st_out = nullptr; void* lo_io = nullptr;     // producer (lo_io: EPI_RESID_SPLIT's lo plane)
  int planes_other = 0;                                                         // producer: write the planes in the other 16-bit format
};
// plipmi_encode_tower_outputs / plipmi_encode_attention_summary: what run_layers hands out per block (fp32, the call's B samples;
// nullptr = not asked for)
struct Taps {
  float* hidden = nullptr;   // [L+1, B, S, D]: slot l+1 after block l (slot 0, the embeddings, is the caller's)
  float* probs = nullptr;    // [L, B, H, S, S]: block l's attention probabilities (attention_probs.hip)
  // attention_summary.hip: the pooled query row of every head, and the rollout R_l = (1/2 mean_h P_l + 1/2 I) R_{l-1} ping-ponged
  // between two buffers (block l writes rollout[l & 1] and reads the other one; block 0 reads the identity)
  float* pooled_rows = nullptr;             // [L, B, H, S]
  float* rollout[2] = {nullptr, nullptr};   // [B, S, S] each
  const int* row_idx = nullptr;             // [B]: the pooled row of each sample (launch_pooled_row_index)
  bool attention() const { return probs || pooled_rows || rollout[0]; }   // something reads the block's qkv activation
};

// One tower forward being enqueued: B samples on stream s.
struct Forward {
  plipmi_engine* e;
  const Model& md;
  const TowerModel& m;
  Tower& t;
  const bool vision;
  const int B;
  hipStream_t s;
  const int causal;              // the text tower's attention is causal
  const int64_t* key_mask;
  // latency path: the batch is small (<= plipmi_engine::latency_batch samples), so every GEMM of the tower takes the split-K
  // small-M kernel instead of walking K serially on a handful of big tiles
  bool small = false;
  // Packed captions (opt-in): the tower is causal and only the EOS row is pooled, so rows past EOS cannot reach the output;
  // they are left out of every kernel.  Needs the pooled last block (no every-token consumer) and the bf16 MFMA attention.
  bool packed = false;
  // `cur` = the operand type of the block being enqueued (what run_gemm / attention launch with); `planes` = the split format the
  // residual planes {h, lo} currently hold: a block whose type differs re-codes them first (enter_block).  The embedding kernels
  // emit the planes in the first block's format.
  int cur, planes;
  const Taps* taps = nullptr;

  enum Regime { kEncode, kEveryToken };   // kEveryToken: big tiles, unpacked rows (plipmi_encode_tower_outputs)
  Forward(plipmi_engine* e_, int tower, int B_, const int64_t* mask, hipStream_t s_, Regime r, bool may_pack)
      : e(e_), md(*e_->model), m(tower == PLIPMI_VISION ? md.vis : md.txt), t(tower == PLIPMI_VISION ? e_->vis : e_->txt),
        vision(tower == PLIPMI_VISION), B(B_), s(s_), causal(vision ? 0 : 1), key_mask(mask), cur(m.layer_dtype(0)), planes(cur) {
    small = r == kEncode && e->half() && B <= e->latency_batch;
    packed = may_pack && !vision && e->text_pack && md.ln_fold && md.pooled_last && e->attn_impl_txt == 1 && t.S <= 128;
  }
  int M() const { return B * t.S; }
  int attn_impl() const { return vision ? e->attn_impl_vis : e->attn_impl_txt; }
  const int* cu() const { return packed ? t.cu : nullptr; }          // packed captions: row offsets / live-row count on the device
  const int* m_dev() const { return packed ? t.mdev : nullptr; }
  LnArgs ln_use(const float* stats) const {
    LnArgs a; a.stats = stats; a.ns = m.D / kLnSlice; a.inv_d = 1.0f / (float)m.D; a.eps = md.cfg.layer_norm_eps;
    return a;
  }
};

// "kernel name|role": the profile keeps the launches of one kernel symbol apart by what they compute (out-proj and fc2
// share a symbol but not a roofline: one is HBM-bound, the other MFMA-bound); bench.py merges them back per symbol.
const char* name_with_role(const char* name, const char* role) {
  static thread_local std::map<std::pair<const char*, const char*>, std::string> cache;
  std::string& v = cache[std::make_pair(name, role)];
  if (v.empty()) v = std::string(name) + "|" + role;
  return v.c_str();
}

// rows = the row count the launch is sized for: the tower's M, or B on the pooled rows (m_dev: packed rows, counted on the device)
int run_gemm(Forward& f, int epi, const void* A, const void* W, void* C, const float* bias, int M, int N, int K,
             int ldc, int np, const char* role, const LnArgs* ln = nullptr, const int* m_dev = nullptr) {
  plipmi_engine* e = f.e;
  GemmParams p = make_params(A, W, C, bias, M, N, K, K, K, ldc);
  p.m_dev = m_dev; p.np = np;
  if (ln) {
    p.ln_stats = ln->stats; p.ln_ns = ln->ns; p.ln_inv_d = ln->inv_d; p.ln_eps = ln->eps;
    p.xb_out = ln->xb_out; p.st_out = ln->st_out; p.lo_io = ln->lo_io; p.planes_other = ln->planes_other;
  }
  bool skinny = role[0] == '~';     // '~role': pooled-row GEMM of the last block -> the small-M split-K kernel when it fits
  if (skinny) ++role;
  skinny = skinny || (f.small && !m_dev);   // latency path: the whole tower of a small batch (packed rows keep the big kernels)
  const char* name = "gemm_nt";
  // algorithmic bytes: operands once, output once (bf16 outputs 2 B, residual read + written -- as one fp32 array or as the 16 + 8-bit
  // 16-bit planes --, + bf16 copy when EPI_RESID_EMIT writes one)
  const double out_bytes = epi_is_colwise(epi) ? (double)M * N * f.md.esz
                           : (double)M * N * (epi == EPI_RESID_SPLIT ? 6.0 : epi_is_resid(epi) ? 8.0 : 4.0) + (epi == EPI_RESID_EMIT ? (double)M * N * 2.0 : 0.0);
  Scope sc(e, f.s, name, 2.0 * M * N * (double)K, ((double)M * K + (double)N * K) * f.md.esz + out_bytes);
  const int rc = (skinny && e->half() && gemm_skinny_supports(epi, M, N, K))
                     ? gemm_launch_skinny(f.cur, epi, p, f.s, &name)
                     : gemm_launch(f.cur, epi, -1, p, f.s, &name);
  if (e->prof.on) sc.rename(name_with_role(name, role));
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "gemm launch (%s, M=%d N=%d K=%d) failed: %s", name, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

// Block l is about to be enqueued: launch with its operand type and, on a LayerNorm-folded engine, make the residual planes
// speak it (hi IS the block's A operand).  On the big-tile path the predecessor's fc2 epilogue already wrote the planes in this block's
// format (GemmParams.planes_other); otherwise (the small-M path) they are re-coded in place: joined in the old code, split in the new
// one -- one more rounding of the 8-bit remainder (common.h split_f32), the new hi = the value correctly rounded to the new operand type.
int enter_block(Forward& f, int l) {
  f.cur = f.m.layer_dtype(l);
  if (f.md.ln_fold && f.planes != f.cur) {
    Scope sc(f.e, f.s, "recode_planes", 0, (double)f.M() * f.m.D * 6);
    HIP_TRY(launch_recode_planes(f.t.h, f.t.lo, (size_t)f.M(), f.m.D, f.planes, f.cur, f.s));
    f.planes = f.cur;
  }
  return PLIPMI_OK;
}

// Attention of the block whose q/k/v GEMM just wrote t.qkv -> t.att; tap >= 0: block `tap`'s probabilities and / or their summaries
// first, as the call's Taps ask (unpacked rows only)
int run_attention(Forward& f, int tap) {
  const Tower& t = f.t;
  const int H = f.m.H, S = t.S, B = f.B, hd = f.m.head();
  const Taps* taps = tap >= 0 ? f.taps : nullptr;
  if (taps && taps->probs) {
    Scope sc(f.e, f.s, "attention_probs", 2.0 * B * H * (double)S * S * hd, (double)B * H * S * S * 4);
    HIP_TRY(launch_attention_probs(t.qkv, taps->probs + (size_t)tap * B * H * S * S, f.cur, B, S, H, hd, f.causal, f.key_mask, f.s));
  }
  // (with a rollout in the same call, its step stores the pooled rows on its way: the tile that holds them forms them anyway)
  if (taps && taps->pooled_rows && !taps->rollout[0]) {
    Scope sc(f.e, f.s, "attention_pooled_rows", 2.0 * B * H * (double)S * hd, (double)B * H * S * (4 + 2.0 * hd * f.md.esz));
    HIP_TRY(launch_attention_pooled_rows(t.qkv, taps->row_idx, taps->pooled_rows + (size_t)tap * B * H * S, f.cur, B, S, H, hd, f.causal,
                                         f.key_mask, f.s));
  }
  if (taps && taps->rollout[0]) {
    Scope sc(f.e, f.s, "attention_rollout_step", 2.0 * B * H * (double)S * S * hd + 2.0 * B * (double)S * S * S,
             (double)B * S * (2.0 * H * hd * f.md.esz + 8.0 * S));
    HIP_TRY(launch_attention_rollout_step(t.qkv, tap == 0 ? nullptr : taps->rollout[(tap - 1) & 1], taps->rollout[tap & 1], f.cur, B, S, H,
                                          hd, f.causal, f.key_mask, f.s, taps->row_idx,
                                          taps->pooled_rows ? taps->pooled_rows + (size_t)tap * B * H * S : nullptr));
  }
  const int impl = f.attn_impl();
  Scope sc(f.e, f.s, impl ? "attention_mfma" : "attention_valu", 4.0 * B * H * (double)S * S * hd, (double)f.M() * 4 * f.m.D * f.md.esz);
  HIP_TRY(launch_attention(t.qkv, t.att, f.cur, B, S, H, hd, f.causal, f.key_mask, impl, f.s, f.cu()));
  return PLIPMI_OK;
}

// LayerNorm-folded q/k/v projection + attention of one block: ONE kernel where the sequence fits the fused tile (77-token
// captions: qkv_attention.hip, the `qkv` activation never reaches memory), else the GEMM and the attention kernel.
// Either way t.att holds the attention output afterwards, the same bits.
int run_qkv_attention(Forward& f, const LayerW& w, const LnArgs& use, int tap = -1) {
  Tower& t = f.t;
  const int M = f.M(), D = f.m.D, H = f.m.H, B = f.B;
  if (tap < 0 && g_fuse_qkv_attention && f.attn_impl() == 1 && !f.packed && !f.small && qkv_attention_supports(f.cur, B, t.S, H, D) &&
      (g_fuse_qkv_attention == 2 || qkv_attention_pays(B, H, gemm_num_cus()))) {
    Scope sc(f.e, f.s, "qkv_attention", 2.0 * M * 3.0 * D * (double)D + 4.0 * B * H * (double)t.S * t.S * f.m.head(), ((double)M * D * 2 + 3.0 * D * D) * f.md.esz);
    HIP_TRY(launch_qkv_attention(f.cur, t.h, w.wqkv, w.bqkv, use.stats, use.inv_d, use.eps, t.att, B, t.S, H, f.causal, f.key_mask, f.s));
    return PLIPMI_OK;
  }
  RUN(run_gemm(f, EPI_BIAS_LN, t.h, w.wqkv, t.qkv, w.bqkv, M, 3 * D, D, 3 * D, 0, "qkv", &use, f.m_dev()));
  return run_attention(f, tap);
}

// n_layers pre-LN residual blocks over the tower's residual stream x (CLIPEncoderLayer, modeling_clip.py:362-383)
int run_layers(Forward& f, int n_layers, bool more_follow = false) {
  plipmi_engine* e = f.e;
  Tower& t = f.t;
  const int M = f.M(), D = f.m.D, F = f.m.F;
  hipStream_t s = f.s;
  auto tap_of = [&](int l) { return f.taps && f.taps->attention() ? l : -1; };
  auto hidden_of = [&](int l) -> float* { return f.taps && f.taps->hidden ? f.taps->hidden + (size_t)(l + 1) * M * D : nullptr; };
  const float eps = f.md.cfg.layer_norm_eps;
  const int* md = f.m_dev();
  if (f.md.ln_fold) {
    // LayerNorm never runs as a pass: the residual stream x = {t.h, t.lo} (operand-type plane + 8-bit remainder plane) and
    // t.st = the rows' statistics partials come from x's producer (embedding kernel, or the residual GEMM's epilogue); the
    // consuming GEMMs read the bf16 plane as their A operand, carry LayerNorm's gain, centring and bias in their weights and
    // apply rstd in their epilogues.  HF order (modeling_clip.py:370-381) is unchanged:
    // x += out_proj(attn(LN1(x))); x += fc2(act(fc1(LN2(x)))), act = the tower's QuickGELU or GELU.
    const LnArgs use = f.ln_use(t.st);
    LnArgs emit; emit.xb_out = t.h; emit.st_out = t.st; emit.lo_io = t.lo;
    for (int l = 0; l < n_layers; ++l) {
      const LayerW& w = f.m.layers[l];
      RUN(enter_block(f, l));
      RUN(run_qkv_attention(f, w, use, tap_of(l)));
      RUN(run_gemm(f, EPI_RESID_SPLIT, t.att, w.wo, nullptr, w.bo, M, D, D, D, 0, "out_proj", &emit, md));
      RUN(run_gemm(f, f.m.fc1_epi(true), t.h, w.w1, t.mlp, w.b1, M, F, D, F, 0, "fc1", &use, md));
      // a block whose successor runs on the other 16-bit operand type (the last f16 block of a mixed text tower) writes its
      // planes in the successor's format from fc2's epilogue -- no re-coding pass over the stream (the tiled kernels only:
      // the small-M kernel of the latency path keeps the separate pass, enter_block)
      const int next_dt = l + 1 < f.m.L ? f.m.layer_dtype(l + 1) : f.cur;
      LnArgs emit2 = emit;
      emit2.planes_other = (next_dt != f.cur && !(f.small && !md)) ? 1 : 0;
      RUN(run_gemm(f, EPI_RESID_SPLIT, t.mlp, w.w2, nullptr, w.b2, M, D, F, D, 0, "fc2", &emit2, md));
      if (emit2.planes_other) f.planes = next_dt;
      if (float* hs = hidden_of(l)) {
        Scope sc(e, s, "join_planes", 0, (double)M * D * 7);
        HIP_TRY(launch_join_planes(t.h, t.lo, hs, (size_t)M, D, f.planes, s));
      }
    }
    if (!more_follow) {
      if (f.packed) return fail(PLIPMI_ERR_INVALID, "packed rows have no every-token form");   // a consumer of plain fp32 rows follows (the every-token head, plipmi_debug_hidden)
      Scope sc(e, s, "join_planes", 0, (double)M * D * 7);
      HIP_TRY(launch_join_planes(t.h, t.lo, t.x, (size_t)M, D, f.planes, s));
    }
    return PLIPMI_OK;
  }
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = f.m.layers[l];
    RUN(enter_block(f, l));
    { Scope sc(e, s, "layernorm", 0, (double)M * D * (4 + f.md.esz));
      HIP_TRY(launch_layernorm(t.x, D, w.ln1w, w.ln1b, t.h, f.cur, M, D, eps, s)); }
    RUN(run_gemm(f, EPI_BIAS, t.h, w.wqkv, t.qkv, w.bqkv, M, 3 * D, D, 3 * D, 0, "qkv"));
    RUN(run_attention(f, tap_of(l)));
    RUN(run_gemm(f, EPI_BIAS_RESID, t.att, w.wo, t.x, w.bo, M, D, D, D, 0, "out_proj"));
    { Scope sc(e, s, "layernorm", 0, (double)M * D * (4 + f.md.esz));
      HIP_TRY(launch_layernorm(t.x, D, w.ln2w, w.ln2b, t.h, f.cur, M, D, eps, s)); }
    RUN(run_gemm(f, f.m.fc1_epi(false), t.h, w.w1, t.mlp, w.b1, M, F, D, F, 0, "fc1"));
    RUN(run_gemm(f, EPI_BIAS_RESID, t.mlp, w.w2, t.x, w.b2, M, D, F, D, 0, "fc2"));
    if (float* hs = hidden_of(l)) HIP_TRY(hipMemcpyAsync(hs, t.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
  }
  return PLIPMI_OK;
}

// The last block on the pooled rows only.  CLIPModel.get_image_features / get_text_features (modeling_clip.py:683-753) hand
// back the projection of ONE row per sample -- CLS after post_layernorm (:650), the EOS row after final_layer_norm
// (:559-581) -- so of the last block's work only q/k/v + attention need every token (keys and values); its out_proj, both
// residual adds, LayerNorm 2, fc1 and fc2 are row-wise and reach the output through that one row.  The reference computes
// them for all 50 / 77 tokens because CLIPModel also returns last_hidden_state, which this path does not.  Results are
// those of the full computation on the pooled rows (same arithmetic, row by row); plipmi_debug_hidden runs the full block.
int run_last_block_pooled(Forward& f, const int64_t* ids, int eos_id) {
  Tower& t = f.t;
  const int D = f.m.D, F = f.m.F, B = f.B;
  const LayerW& w = f.m.layers[f.m.L - 1];
  RUN(enter_block(f, f.m.L - 1));
  RUN(run_qkv_attention(f, w, f.ln_use(t.st)));
  { Scope sc(f.e, f.s, "pool_gather", 0, (double)B * D * (2 * f.md.esz + 8));
    HIP_TRY(launch_pool_gather(t.att, t.h, t.lo, t.S, D, ids, eos_id, t.attp, t.xp, B, f.cur, f.s, f.cu())); }
  LnArgs emit; emit.xb_out = t.hp; emit.st_out = t.stp;
  const LnArgs use = f.ln_use(t.stp);
  RUN(run_gemm(f, EPI_RESID_EMIT, t.attp, w.wo, t.xp, w.bo, B, D, D, D, 0, "~out_proj_pooled", &emit));
  RUN(run_gemm(f, f.m.fc1_epi(true), t.hp, w.w1, t.mlpp, w.b1, B, F, D, F, 0, "~fc1_pooled", &use));
  RUN(run_gemm(f, EPI_BIAS_RESID, t.mlpp, w.w2, t.xp, w.b2, B, D, F, D, 0, "~fc2_pooled"));
  return PLIPMI_OK;
}

// CLIPVisionEmbeddings + pre_layrnorm (modeling_clip.py:202-218,642): x = LN(cat(cls, conv(pixels)) + pos)
int vision_embed(Forward& f, const float* pixels, const uint8_t* tiles_u8) {
  plipmi_engine* e = f.e;
  const Model& md = f.md;
  const plipmi_config& g = md.cfg;
  Tower& t = f.t;
  const int B = f.B, D = f.m.D, dtype = f.m.dtype;
  hipStream_t s = f.s;
  // fp32 pixels, 16-bit engine, 16- / 32-pixel patches: the patch GEMM reads the pixels itself (im2col on load -- four pixels per lane
  // into registers, rounded to the operand type, written to its A stage), no unfold pass and no `patches` round trip.  Same operand
  // bits as the unfold kernel's, hence the same embedding rows.
  // uint8 tiles (round 6): the same gather on the HWC bytes, CLIP normalisation as one fma per pixel -- the rows the unfold_u8 pass +
  // plain patch GEMM produce, bit for bit.
  const bool gather = g_patch_gather && e->half() && !f.small && md.kpad == 3 * g.patch_size * g.patch_size &&
                      gemm_gather_supports(dtype, B, e->img_h, e->img_w, g.patch_size, D);
  const double px_bytes = (double)B * 3 * e->img_h * e->img_w;
  if (!gather) {   // the patch rows [B*np, kpad] first; the launch order of the two forms is the one their profiles were recorded in
    if (tiles_u8) {
      Scope sc(e, s, "unfold_patches_u8", 0, px_bytes + (double)B * e->np * md.kpad * md.esz);
      HIP_TRY(launch_unfold_patches_u8(tiles_u8, e->patches, dtype, B, e->img_h, e->img_w, g.patch_size, md.kpad, s));
    } else {
      Scope sc(e, s, "unfold_patches", 0, px_bytes * 4 + (double)B * e->np * md.kpad * md.esz);
      HIP_TRY(launch_unfold_patches(pixels, e->patches, dtype, B, e->img_h, e->img_w, g.patch_size, md.kpad, s));
    }
  }
  { Scope sc(e, s, "cls_rows", 0, (double)B * D * 4);
    HIP_TRY(launch_cls_rows(md.cls, e->vpos, t.x, B, t.S, D, s)); }
  if (gather) {
    GemmParams p = make_params(nullptr, md.patch_w, t.x, e->vpos, B * e->np, D, md.kpad, md.kpad, md.kpad, D);
    p.np = e->np;
    p.pix = pixels; p.tiles = tiles_u8; p.img_h = e->img_h; p.img_w = e->img_w; p.patch_log2 = g.patch_size == 32 ? 5 : 4;
    const char* name = "gemm_nt";
    Scope sc(e, s, name, 2.0 * p.M * p.N * (double)p.K, px_bytes * (tiles_u8 ? 1 : 4) + (double)p.N * p.K * md.esz + (double)p.M * p.N * 4);
    const int rc = gemm_launch_gather(dtype, p, s, &name);
    if (e->prof.on) sc.rename(name_with_role(name, "patch_embed"));
    if (rc != 0) return fail(PLIPMI_ERR_HIP, "patch GEMM (im2col on load) failed: %s", hipGetErrorString((hipError_t)rc));
  } else {
    RUN(run_gemm(f, EPI_PATCH, e->patches, md.patch_w, t.x, e->vpos, B * e->np, D, md.kpad, D, e->np, "patch_embed"));
  }
  if (md.ln_fold) {   // the tower's one LayerNorm pass: fp32 embedding rows in, the split residual stream + row statistics out
    Scope sc(e, s, "layernorm", 0, (double)B * t.S * D * 8.2);
    HIP_TRY(launch_layernorm_emit(t.x, md.pre_w, md.pre_b, t.h, t.lo, t.st, B * t.S, D, g.layer_norm_eps, dtype, s));
    return PLIPMI_OK;
  }
  { Scope sc(e, s, "layernorm", 0, (double)B * t.S * D * 8);
    HIP_TRY(launch_layernorm(t.x, D, md.pre_w, md.pre_b, t.x, 0, B * t.S, D, g.layer_norm_eps, s)); }
  return PLIPMI_OK;
}

int text_embed(Forward& f, const int64_t* ids, int eos_id) {
  plipmi_engine* e = f.e;
  const Model& md = f.md;
  Tower& t = f.t;
  const int B = f.B, D = f.m.D, vocab = md.cfg.vocab_size;
  hipStream_t s = f.s;
  if (f.packed) {
    { Scope sc(e, s, "text_pack", 0, (double)B * t.S * 12);
      HIP_TRY(launch_text_pack(ids, B, t.S, eos_id, t.cu, t.rowmap, t.mdev, s)); }
    Scope sc(e, s, "text_embed", 0, (double)B * t.S * D * 8.2);
    HIP_TRY(launch_text_embed_emit_packed(ids, md.tok, md.tpos, t.h, t.lo, t.st, t.rowmap, t.mdev, B * t.S, t.S, D,
                                          vocab, e->bad_id, f.planes, s));
    return PLIPMI_OK;
  }
  Scope sc(e, s, "text_embed", 0, (double)B * t.S * D * (md.ln_fold ? 8.2 : 8.0));
  if (md.ln_fold) HIP_TRY(launch_text_embed_emit(ids, md.tok, md.tpos, t.h, t.lo, t.st, B, t.S, D, vocab, e->bad_id, f.planes, s));
  else HIP_TRY(launch_text_embed(ids, md.tok, md.tpos, t.x, B, t.S, D, vocab, e->bad_id, s));
  return PLIPMI_OK;
}

// the tower's input rows: pixels (fp32) or tiles (uint8) for the vision tower, token ids for the text tower
int embed(Forward& f, const void* input, bool input_u8, int eos_id) {
  if (!f.vision) return text_embed(f, reinterpret_cast<const int64_t*>(input), eos_id);
  return vision_embed(f, input_u8 ? nullptr : reinterpret_cast<const float*>(input), input_u8 ? reinterpret_cast<const uint8_t*>(input) : nullptr);
}

// pooled row -> LayerNorm -> bias-free projection (-> L2 normalise): row `ids`' EOS position (nullptr: row 0) of every S rows of x.
// Widths that are multiples of 32 (every config plipmi_create accepts today) run the projection on the split-K exact-fp32 MFMA
// head kernel; the fused one-block-per-sample kernel covers anything else.
int run_head(Forward& f, const float* x, int S, const int64_t* ids, int eos_id, float* out, int normalize) {
  plipmi_engine* e = f.e;
  const TowerModel& m = f.m;
  const int P = f.md.cfg.projection_dim, D = m.D, B = f.B;
  const float eps = f.md.cfg.layer_norm_eps;
  hipStream_t s = f.s;
  if (P % 32 == 0 && D % 32 == 0) {
    { Scope sc(e, s, "pool_layernorm", 0, (double)B * D * 8);
      HIP_TRY(launch_pool_layernorm(x, S, D, ids, eos_id, m.head_ln_w, m.head_ln_b, eps, f.t.pooled, B, s)); }
    { Scope sc(e, s, "head_gemm", 2.0 * B * P * (double)D, ((double)B * D + (double)P * D + (double)B * P) * 4);
      HIP_TRY(launch_head_gemm(f.t.pooled, m.proj, out, B, P, D, s)); }
    if (normalize) { Scope sc(e, s, "l2_normalize", 0, (double)B * P * 8); HIP_TRY(launch_l2_normalize(out, B, P, s)); }
    return PLIPMI_OK;
  }
  Scope sc(e, s, "pool_head", 2.0 * B * D * P, (double)D * P * 4);
  HIP_TRY(launch_pool_head(x, S, D, ids, eos_id, m.head_ln_w, m.head_ln_b, eps, m.proj_t, P, out, B, normalize, s));
  return PLIPMI_OK;
}

// One tower's embedding forward on whatever pointers it is given (the caller's, or the staging buffers under capture):
// embed, the blocks, the head.  The text tower pools each caption's EOS row (found from its ids), the vision tower row 0.
int tower_forward(plipmi_handle h, int tower, const void* input, bool input_u8, const int64_t* mask, int B, int eos_id, float* out,
                  int normalize, hipStream_t s) {
  Forward f(h, tower, B, mask, s, Forward::kEncode, /*may_pack=*/true);
  const int64_t* ids = f.vision ? nullptr : reinterpret_cast<const int64_t*>(input);
  if (f.vision) eos_id = -1;
  RUN(embed(f, input, input_u8, eos_id));
  if (f.md.pooled_last) {
    RUN(run_layers(f, f.m.L - 1, /*more_follow=*/true));
    RUN(run_last_block_pooled(f, ids, eos_id));
    return run_head(f, f.t.xp, 1, nullptr, -1, out, normalize);
  }
  RUN(run_layers(f, f.m.L));
  return run_head(f, f.t.x, f.t.S, ids, eos_id, out, normalize);
}

// Small batches: replay a captured graph of the same launches.  kind 0 = fp32 pixels, 1 = uint8 tiles, 2 = text.
// Call 1 of a shape runs eagerly (and leaves every kernel's attributes set), call 2 captures, later calls replay.
template <typename Fwd>
int graph_or_eager(plipmi_handle h, int kind, int B, int normalize, int eos, hipStream_t s, const void* in, size_t in_bytes,
                   void* in_stage, const int64_t* mask, size_t mask_bytes, float* out, float* out_stage,
                   Fwd&& forward /* (in, mask, B, out, stream) -> rc */) {
  const bool eligible = h->graph_batch > 0 && B <= h->graph_batch && !h->prof.on;
  if (!eligible) return forward(in, mask, B, out, s);
  const int has_mask = mask != nullptr;
  GraphEntry& ge = h->graphs.at(std::make_tuple(kind, B, normalize, eos, has_mask));
  if (ge.seen++ == 0) return forward(in, mask, B, out, s);
  HIP_TRY(hipMemcpyAsync(in_stage, in, in_bytes, hipMemcpyDeviceToDevice, s));
  if (has_mask) HIP_TRY(hipMemcpyAsync(h->g_tmask, mask, mask_bytes, hipMemcpyDeviceToDevice, s));
  if (!ge.exec) {
    hipGraph_t graph = nullptr;
    hipStream_t cap = nullptr;
    HIP_TRY(h->graphs.capture_stream(&cap));
    HIP_TRY(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    const int rc = forward(in_stage, has_mask ? h->g_tmask : nullptr, B, out_stage, cap);
    const hipError_t ee = hipStreamEndCapture(cap, &graph);   // always end the capture: the stream must leave capture mode
    if (rc != PLIPMI_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    if (ee != hipSuccess) return fail(PLIPMI_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ee));
    const hipError_t ie = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (ie != hipSuccess) { ge.exec = nullptr; return fail(PLIPMI_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie)); }
  }
  HIP_TRY(hipGraphLaunch(ge.exec, s));
  HIP_TRY(hipMemcpyAsync(out, out_stage, (size_t)B * h->cfg().projection_dim * 4, hipMemcpyDeviceToDevice, s));
  return PLIPMI_OK;
}

// What the three encode entries share: the argument checks, the split into passes (plipmi_config.pass_batch) and the small-batch
// graph replay.  `in`: B samples of `stride` bytes each; kind / in_stage / out_stage: the graph's key and staging buffers;
// forward(in, mask, B, out, stream) enqueues one tower forward.
template <typename Fwd>
int encode(plipmi_handle h, const void* in, size_t stride, const char* null_msg, int kind, void* in_stage, float* out_stage,
           const int64_t* mask, int B, int eos, float* out, int normalize, void* stream, Fwd&& forward) {
  if (B == 0) return PLIPMI_OK;
  if (!in || !out) return fail(PLIPMI_ERR_INVALID, "%s", null_msg);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t mask_stride = (size_t)h->cfg().context_length;
  if (const int n = passes_of(h->pass_batch, B); n > 1) {
    for (int b0 = 0, i = 0; i < n; ++i) {
      const int nb = pass_rows(B, n, i);
      RUN(forward(reinterpret_cast<const char*>(in) + (size_t)b0 * stride, mask ? mask + (size_t)b0 * mask_stride : nullptr, nb,
                  out + (size_t)b0 * h->cfg().projection_dim, s));
      b0 += nb;
    }
    return PLIPMI_OK;
  }
  return graph_or_eager(h, kind, B, normalize != 0, eos, s, in, (size_t)B * stride, in_stage, mask, (size_t)B * mask_stride * 8, out,
                        out_stage, forward);
}

}  // namespace

extern "C" {

int plipmi_encode_image(plipmi_handle h, const float* pixels, int B, float* out, int normalize, void* stream) {
  RUN(check_batch(h, B));
  return encode(h, pixels, (size_t)3 * h->img_h * h->img_w * 4, "null pixels/out", 0, h->g_vin, h->g_vout, nullptr, B, 0, out, normalize, stream,
                [&](const void* in, const int64_t*, int nb, float* o, hipStream_t st) {
                  return tower_forward(h, PLIPMI_VISION, in, false, nullptr, nb, -1, o, normalize, st); });
}

int plipmi_encode_image_u8(plipmi_handle h, const uint8_t* tiles, int B, float* out, int normalize, void* stream) {
  RUN(check_batch(h, B));
  return encode(h, tiles, (size_t)3 * h->img_h * h->img_w, "null tiles/out", 1, h->g_vin, h->g_vout, nullptr, B, 0, out, normalize, stream,
                [&](const void* in, const int64_t*, int nb, float* o, hipStream_t st) {
                  return tower_forward(h, PLIPMI_VISION, in, true, nullptr, nb, -1, o, normalize, st); });
}

int plipmi_encode_text(plipmi_handle h, const int64_t* ids, const int64_t* attention_mask, int B, int eos_token_id,
                       float* out, int normalize, void* stream) {
  RUN(check_batch(h, B));
  RUN(check_async(h));
  return encode(h, ids, (size_t)h->cfg().context_length * 8, "null ids/out", 2, h->g_tin, h->g_tout, attention_mask, B, eos_token_id, out,
                normalize, stream, [&](const void* in, const int64_t* m, int nb, float* o, hipStream_t st) {
                  return tower_forward(h, PLIPMI_TEXT, in, false, m, nb, eos_token_id, o, normalize, st); });
}

int plipmi_debug_hidden(plipmi_handle h, int tower, int layer, const void* input, int B, float* out, void* stream) {
  RUN(check_batch(h, B));
  if (B == 0) return PLIPMI_OK;
  if (!input || !out) return fail(PLIPMI_ERR_INVALID, "null input/out");
  if (!valid_tower(tower)) return fail(PLIPMI_ERR_INVALID, "tower must be 0 or 1");
  Forward f(h, tower, B, nullptr, reinterpret_cast<hipStream_t>(stream), Forward::kEncode, /*may_pack=*/false);
  if (layer < 0 || layer > f.m.L) return fail(PLIPMI_ERR_INVALID, "layer %d outside [0,%d]", layer, f.m.L);
  RUN(embed(f, input, false, -1));
  RUN(run_layers(f, layer));
  HIP_TRY(hipMemcpyAsync(out, f.t.x, (size_t)B * f.t.S * f.m.D * 4, hipMemcpyDeviceToDevice, f.s));
  return PLIPMI_OK;
}

// The per-token outputs of one tower (CLIPVisionTransformer / CLIPTextTransformer with output_hidden_states /
// output_attentions): eager, every block dense on every token, text unpacked and through the q/k/v GEMM + attention pair
// (the probabilities need `qkv` in memory).  Its regime is the call's own (Forward::kEveryToken): the handle's packing, fusion rule,
// captured graphs and latency setting are read by the encode paths as before, and the workspace they use is rewritten by their next call.
int plipmi_encode_tower_outputs(plipmi_handle h, int tower, const void* input, const int64_t* attention_mask, int B, int eos_token_id,
                                float* last_hidden, float* pooled, float* hidden_states, float* attentions, void* stream) {
  RUN(check_batch(h, B));
  if (!valid_tower(tower)) return fail(PLIPMI_ERR_INVALID, "tower must be 0 (vision) or 1 (text), got %d", tower);
  const bool vision = tower == PLIPMI_VISION;
  if (!vision) RUN(check_async(h));
  if (B == 0) return PLIPMI_OK;
  if (!input) return fail(PLIPMI_ERR_INVALID, "null input");
  if (!last_hidden && !pooled && !hidden_states && !attentions) return fail(PLIPMI_ERR_INVALID, "no output buffer given");
  if (vision && attention_mask) return fail(PLIPMI_ERR_INVALID, "the vision tower takes no attention mask");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Forward f(h, tower, B, attention_mask, s, Forward::kEveryToken, /*may_pack=*/false);
  Taps taps;
  taps.hidden = hidden_states;
  taps.probs = attentions;
  f.taps = &taps;
  Tower& t = f.t;
  const int M = f.M(), D = f.m.D;
  const float eps = h->cfg().layer_norm_eps;
  const int64_t* ids = vision ? nullptr : reinterpret_cast<const int64_t*>(input);
  RUN(embed(f, input, false, -1));
  if (hidden_states) {  // hidden_states[0]: the embeddings (vision: after pre_layrnorm)
    if (f.md.ln_fold) {
      Scope sc(h, s, "join_planes", 0, (double)M * D * 7);
      HIP_TRY(launch_join_planes(t.h, t.lo, hidden_states, (size_t)M, D, f.planes, s));
    } else {
      HIP_TRY(hipMemcpyAsync(hidden_states, t.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    }
  }
  RUN(run_layers(f, f.m.L));   // t.x = the encoder output, fp32
  if (last_hidden) {
    if (vision) {
      HIP_TRY(hipMemcpyAsync(last_hidden, t.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    } else {
      Scope sc(h, s, "layernorm", 0, (double)M * D * 8);
      HIP_TRY(launch_layernorm(t.x, D, f.m.head_ln_w, f.m.head_ln_b, last_hidden, 0, M, D, eps, s));
    }
  }
  if (pooled) {
    Scope sc(h, s, "pool_layernorm", 0, (double)B * D * 8);
    HIP_TRY(launch_pool_layernorm(t.x, t.S, D, ids, vision ? -1 : eos_token_id, f.m.head_ln_w, f.m.head_ln_b, eps, pooled, B, s));
  }
  return PLIPMI_OK;
}

// The attention summaries of one tower (include/plipmi.h): the walk of plipmi_encode_tower_outputs -- eager, every block dense on every
// token, q/k/v GEMM + attention as two kernels -- with the summary kernels (attention_summary.hip) tapping each block's qkv activation.
// The pooled-row indices and the rollout's ping-pong buffers live in handle scratch of their own (summary_ws), outside the tower
// workspace; a caller's rollout_matrix serves as the buffer the last block writes.
int plipmi_encode_attention_summary(plipmi_handle h, int tower, const void* input, const int64_t* attention_mask, int B, int eos_token_id,
                                    float* pooled_attention, float* rollout, float* rollout_matrix, void* stream) {
  RUN(check_batch(h, B));
  if (!valid_tower(tower)) return fail(PLIPMI_ERR_INVALID, "tower must be 0 (vision) or 1 (text), got %d", tower);
  const bool vision = tower == PLIPMI_VISION;
  if (!vision) RUN(check_async(h));
  if (B == 0) return PLIPMI_OK;
  if (!input) return fail(PLIPMI_ERR_INVALID, "null input");
  if (!pooled_attention && !rollout && !rollout_matrix) return fail(PLIPMI_ERR_INVALID, "no output buffer given");
  if (vision && attention_mask) return fail(PLIPMI_ERR_INVALID, "the vision tower takes no attention mask");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Forward f(h, tower, B, attention_mask, s, Forward::kEveryToken, /*may_pack=*/false);
  const int S = f.t.S, L = f.m.L;
  const bool roll = rollout || rollout_matrix;
  // scratch: rows [B] int32, then the rollout buffers the caller did not bring (one beside a rollout_matrix, else two)
  const size_t rows_bytes = align_up((size_t)B * sizeof(int), 256), r_bytes = align_up((size_t)B * S * S * sizeof(float), 256);
  const int own = roll ? (rollout_matrix ? 1 : 2) : 0;
  RUN(h->summary_ws.reserve(rows_bytes + own * r_bytes, s));
  int* rows = reinterpret_cast<int*>(h->summary_ws.data());
  float* r0 = reinterpret_cast<float*>(h->summary_ws.data() + rows_bytes);
  Taps taps;
  taps.pooled_rows = pooled_attention;
  taps.row_idx = rows;
  if (roll) {
    const int last = (L - 1) & 1;               // the buffer block L-1 writes
    taps.rollout[last] = rollout_matrix ? rollout_matrix : r0 + r_bytes / sizeof(float);
    taps.rollout[last ^ 1] = r0;
  }
  f.taps = &taps;
  const int64_t* ids = vision ? nullptr : reinterpret_cast<const int64_t*>(input);
  { Scope sc(h, s, "pooled_row_index", 0, (double)B * (vision ? 4 : S * 8));
    HIP_TRY(launch_pooled_row_index(ids, S, vision ? -1 : eos_token_id, rows, B, s)); }
  RUN(embed(f, input, false, -1));
  RUN(run_layers(f, L));
  if (rollout) {
    Scope sc(h, s, "attention_rollout_row", 0, (double)B * S * 8);
    HIP_TRY(launch_attention_rollout_row(taps.rollout[(L - 1) & 1], rows, rollout, B, S, s));
  }
  return PLIPMI_OK;
}

// Dense image-text similarity (include/plipmi.h): the vision walk of plipmi_encode_tower_outputs, then the pooled head's arithmetic on
// EVERY row -- post_layernorm, the fp32 projection -- and the scores kernel (token_scores.hip).  The LayerNorm'd rows and an E nobody
// asked for live in handle scratch of their own (token_ws), outside the tower workspace.
int plipmi_encode_token_similarity(plipmi_handle h, const float* pixels, int B, const float* text_embeds, int C, float scale, int softmax,
                                   float* token_embeds, float* similarity, void* stream) {
  static_assert(PLIPMI_TOKEN_SIM_MAX_C == kTokenSimMaxC, "the header's limit is the kernel's");
  RUN(check_batch(h, B));
  if (C < 1 || C > PLIPMI_TOKEN_SIM_MAX_C) return fail(PLIPMI_ERR_INVALID, "C = %d text rows: 1 .. %d", C, PLIPMI_TOKEN_SIM_MAX_C);
  if (B == 0) return PLIPMI_OK;
  if (!pixels) return fail(PLIPMI_ERR_INVALID, "null pixels");
  if (!text_embeds) return fail(PLIPMI_ERR_INVALID, "null text_embeds");
  if (reinterpret_cast<uintptr_t>(text_embeds) % 16) return fail(PLIPMI_ERR_INVALID, "text_embeds must be 16-byte aligned");
  if (!token_embeds && !similarity) return fail(PLIPMI_ERR_INVALID, "no output buffer given (token_embeds and similarity are both NULL)");
  const int P = h->cfg().projection_dim;
  if (P % 32) return fail(PLIPMI_ERR_INVALID, "projection_dim = %d: the per-token head takes multiples of 32", P);
  if (token_embeds && reinterpret_cast<uintptr_t>(token_embeds) % 16) return fail(PLIPMI_ERR_INVALID, "token_embeds must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Forward f(h, PLIPMI_VISION, B, nullptr, s, Forward::kEveryToken, /*may_pack=*/false);
  const int M = f.M(), D = f.m.D;
  const size_t ln_bytes = align_up((size_t)M * D * sizeof(float), 256);
  RUN(h->token_ws.reserve(ln_bytes + (token_embeds ? 0 : (size_t)M * P * sizeof(float)), s));
  float* ln = reinterpret_cast<float*>(h->token_ws.data());
  float* E = token_embeds ? token_embeds : reinterpret_cast<float*>(h->token_ws.data() + ln_bytes);
  RUN(embed(f, pixels, false, -1));
  RUN(run_layers(f, f.m.L));   // t.x = the encoder output, fp32
  { Scope sc(h, s, "layernorm", 0, (double)M * D * 8);
    HIP_TRY(launch_layernorm(f.t.x, D, f.m.head_ln_w, f.m.head_ln_b, ln, 0, M, D, h->cfg().layer_norm_eps, s)); }
  {
    // one tile for every M (the 128 x 128 one; projections narrower than that: the 32 x 32 tile of the pooled head), so that a row's
    // bits do not depend on the batch it travels in
    const char* name = "head_gemm";
    Scope sc(h, s, name, 2.0 * M * P * (double)D, ((double)M * D + (double)P * D + (double)M * P) * 4);
    if (P % 128 == 0) {
      const GemmParams p = make_params(ln, f.m.proj, E, nullptr, M, P, D, D, D, P);
      const int rc = gemm_launch(PLIPMI_F32, EPI_SCALE, 1, p, s, &name);
      if (rc != 0) return fail(PLIPMI_ERR_HIP, "token projection gemm (M=%d N=%d K=%d) failed: %s", M, P, D, hipGetErrorString((hipError_t)rc));
    } else {
      HIP_TRY(launch_head_gemm(ln, f.m.proj, E, M, P, D, s));
    }
    if (h->prof.on) sc.rename(name_with_role(name, "token_proj"));
  }
  if (similarity) {
    Scope sc(h, s, "token_scores", 2.0 * M * (double)P * (C + 1), ((double)M * P + (double)C * P + (double)M * C) * 4);
    HIP_TRY(launch_token_scores(E, M, P, text_embeds, C, scale, softmax, similarity, s));
  }
  return PLIPMI_OK;
}

}  // extern "C"
