/*
 * plipmi.h -- C ABI of libplipmi.so, the MI355X (gfx950) PLIP embedding engine.
 *
 * This is the drop-in boundary for the one hot path of PathologyFoundation/plip:
 * the batched encode_images / encode_text forward and the image x text
 * cosine-similarity logits.  The reference has no FFI layer of its own -- the
 * seam is "the object stored in self.model" (reference plip.py:18) -- so every
 * entry point below names the reference call it replaces:
 *
 *   plipmi_create         <- CLIPModel.from_pretrained(...).to(device)        plip.py:26,18
 *                            clip.load(arch) + load_state_dict(...)           reproducibility/embedders/factory.py:21-25
 *   plipmi_encode_image   <- self.model.get_image_features(**batch)           plip.py:50
 *                            self.model.encode_image(images)                  reproducibility/embedders/plip.py:48
 *   plipmi_encode_image_u8<- self.preprocess(images=...) + get_image_features           plip.py:32-35,50
 *   plipmi_resize_crop_u8 <- Resize(n_px, bicubic) + CenterCrop(n_px)                  reproducibility/embedders/transform.py:45-48
 *   plipmi_resize_crop_u8_ragged <- the same two steps on images whose sizes differ     transform.py:45-48, plip.py:32-35,
 *                            (CLIPImageDataset: any file through _transform)           reproducibility/dataset_loading/internal_datasets.py:42
 *   plipmi_encode_text    <- self.model.get_text_features(**batch)            plip.py:68
 *                            self.model.encode_text(clip.tokenize(...))       reproducibility/embedders/plip.py:65-66
 *   plipmi_l2_normalize   <- x / np.linalg.norm(x, axis=-1, keepdims=True)    plip.py:75, embedders/plip.py:53,73
 *   plipmi_logits         <- CLIPModel.forward -> logits_per_image/_text      README.md:45-50 (HF modeling_clip.py:810-817)
 *                            image_embeddings.dot(text_embeddings.T); argmax  reproducibility/evaluation/zero_shot/zero_shot.py:12-13
 *   plipmi_topk           <- cosine_sim.argsort()[:, -k:][:, ::-1]            plip.py:78-87, evaluation/retrieval/retrieval.py:13-18
 *   plipmi_similarity_topk<- the same two call sites, fused with the dot product (no [N,N] matrix)
 *   plipmi_probe_fit      <- SGDClassifier(loss="log_loss", ...).fit(train_x, train_y)   reproducibility/evaluation/linear_probing/linear_classifier.py:18-31
 *   plipmi_probe_predict  <- classifier.predict(x)                                       linear_classifier.py:32-33
 *   plipmi_softmax_fit    <- LinearClassifier + nn.CrossEntropyLoss() on a frozen tower         reproducibility/fine_tuning/finetune.py
 *                            (and the CLIP paper's LogisticRegression(C=0.316, max_iter=1000).fit(train_x, train_y))
 *   plipmi_region_select, plipmi_region_gather <- nothing in the reference, which takes tiles somebody has already cut: the grid,
 *                            the background filter and the stacking its users do in numpy in front of encode_images
 *   plipmi_warp_u8        <- RandomCrop + RandomHorizontalFlip + RandomAffine, then RandomPerspective      reproducibility/embedders/transform.py
 *                            (_train_transform; one call per stage, PIL's Image.transform bytes)
 *
 * Conventions
 *   - plain C, no torch / HIP types in the signatures: device buffers are raw
 *     `void*` device addresses (tensor.data_ptr()), the stream is a
 *     hipStream_t passed as `void*` (NULL = the legacy default stream).
 *   - every call only ENQUEUES work on the given stream and returns; the
 *     caller synchronises.  Inputs are never modified; outputs are caller-owned.
 *   - one handle per GPU / process, not thread-safe per handle.
 *   - return value: 0 = OK, anything else = error; the message is available
 *     from plipmi_last_error() (thread local).
 *   - fp32 tensors are row-major C-contiguous; pixel input is NCHW.
 */
#ifndef PLIPMI_H
#define PLIPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLIPMI_VERSION 412 /* (plipmi_tower_shape / plipmi_encode_tower_outputs and plipmi_clone_resolution are new entries, the
                            * config struct is unchanged: the number stays, an existing test pins it)
                            * (PLIPMI_FLAG_VISION_GELU / PLIPMI_FLAG_TEXT_GELU are new bits of `flags`: the struct and the number stay
                            * again; a library built before them refuses the bits with its "unknown bits in plipmi_config.flags"
                            * error, it never runs a gelu checkpoint with QuickGELU)
                            * 0.4.1: `pass_batch` appended to the config struct -- a 0.4.0 caller's shorter struct means 0 = automatic;
                            * 0.4.0: plipmi_config starts with `struct_size` (the struct can grow at its tail without breaking
                            * callers compiled against an older header); test / A-B hooks moved to plipmi_test.h
                            * (0.3.1: `text_f16_layers`, PLIPMI_ERR_TOKEN_ID; 0.3.0: `flags`, `graph_batch`, PLIPMI_F16) */

/* arithmetic the towers' GEMMs and attention run in (accumulation, LayerNorm,
 * softmax statistics, residual stream, projections and logits are always fp32):
 *   PLIPMI_F32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *   PLIPMI_BF16  bf16 MFMA operands (8 significand bits)  -- BASELINE.json configs[2] as named
 *   PLIPMI_F16   IEEE half MFMA operands (11 significand bits, +-65504; outputs saturate), same matrix-core rate as
 *                bf16.  The reference's own GPU path runs its CLIP in this type (OpenAI clip.load on "cuda" ->
 *                convert_weights: reproducibility/embedders/factory.py:21, scripts/extract_embedding.py:94-97).
 * (The experimental fp8-weights mode of earlier versions, value 2, is gone: 2.7e-3 against the 1e-3 cosine bar.) */
enum { PLIPMI_F32 = 0, PLIPMI_BF16 = 1, PLIPMI_F16 = 2 };

/* plipmi_config.flags -- every switch of a handle's behaviour is an argument of plipmi_create (or a per-handle setter
 * below); the library reads no environment variables for them */
enum {
  PLIPMI_FLAG_SEPARATE_LAYERNORM = 1,  /* 16-bit engines: run the 2 x L block LayerNorms as their own kernels instead
                                        * of folding them into the q/k/v and fc1 GEMMs (A/B measurements) */
  PLIPMI_FLAG_DENSE_LAST_BLOCK = 2,    /* compute the last block's out_proj / fc1 / fc2 on every token, as the reference
                                        * does, instead of on the pooled row of each sample only */
  PLIPMI_FLAG_PACK_CAPTIONS = 4,       /* start with caption packing on (plipmi_set_text_packing) */
  PLIPMI_FLAG_VALU_ATTENTION = 8,      /* exact-fp32 VALU attention kernel instead of the MFMA kernels (A/B measurements) */
  PLIPMI_FLAG_TEXT_TOWER_F16 = 16,     /* bf16 engine only: the TEXT tower's operands (weights, activations, its plane of
                                        * the residual stream) are IEEE half instead of bf16.  The text side carries
                                        * 3.2x the image side's embedding error in bf16 (operand rounding of the weights,
                                        * coherent over a caption's tokens) and 40 % of the step's time:
                                        * half precision there buys most of the f16 engine's accuracy for a third of
                                        * its cost.  The image tower stays bf16. */
  PLIPMI_FLAG_VISION_GELU = 32,        /* the vision tower's MLP activation is the exact (erf) GELU of HF hidden_act = "gelu",
                                        * 0.5 x (1 + erf(x / sqrt 2)), instead of QuickGELU (hidden_act = "quick_gelu", the default):
                                        * open_clip / LAION-trained checkpoints.  Every dtype and every path of the engine. */
  PLIPMI_FLAG_TEXT_GELU = 64           /* the same for the text tower; the two towers choose independently */
};

/* towers, for plipmi_debug_hidden */
enum { PLIPMI_VISION = 0, PLIPMI_TEXT = 1 };

/* status codes */
enum {
  PLIPMI_OK = 0,
  PLIPMI_ERR_INVALID = 1,   /* bad argument / unsupported shape */
  PLIPMI_ERR_HIP = 2,       /* a HIP runtime call failed */
  PLIPMI_ERR_NODEVICE = 3,  /* no gfx950 device visible */
  PLIPMI_ERR_NOMEM = 4,
  PLIPMI_ERR_TOKEN_ID = 5,  /* an EARLIER plipmi_encode_text on the handle saw a token id outside the vocabulary (below) */
  PLIPMI_ERR_NOT_CONVERGED = 6  /* plipmi_probe_fit stopped at max_iter (or its line search stalled) above gtol; outputs are valid */
};

typedef struct plipmi_engine* plipmi_handle;

/* Architecture = the numbers in HF CLIPConfig (configuration_clip.py:47-64,97-109).
 * `struct_size` = sizeof(plipmi_config) AS THE CALLER COMPILED IT: plipmi_create reads that many bytes and takes every later
 * member as 0 (= its default), so members appended in later versions do not turn into garbage for older callers; a size
 * smaller than the 0.4.0 struct (through `max_batch`) or larger than the library's own is rejected.
 * Attention head size, per tower: head_dim = width / heads.  64 -- every OpenAI CLIP / PLIP variant -- runs the kernels tuned for it
 * (and only such a text tower takes the fused q/k/v + attention kernel and caption packing).  Any other multiple of 8 from 72 to 128
 * (vision; text: to 120) runs the padded-head attention kernels: open_clip's ViT-H/14 (16 heads of 80) and ViT-g/14 (16 of 88) vision
 * towers.  Everything else is PLIPMI_ERR_INVALID from plipmi_create, with a message that names head_dim. */
typedef struct plipmi_config {
  int32_t struct_size;     /* sizeof(plipmi_config) */
  int32_t image_size;      /* 224 */
  int32_t patch_size;      /* 32  */
  int32_t v_width;         /* 768 */
  int32_t v_layers;        /* 12  */
  int32_t v_heads;         /* 12  (head_dim = v_width / v_heads: 64, or another multiple of 8 up to 128 -- see below) */
  int32_t v_mlp;           /* 3072 */
  int32_t vocab_size;      /* 49408 */
  int32_t context_length;  /* 77 */
  int32_t t_width;         /* 512 */
  int32_t t_layers;        /* 12 */
  int32_t t_heads;         /* 8   (head_dim = t_width / t_heads: 64, or another multiple of 8 up to 120) */
  int32_t t_mlp;           /* 2048 */
  int32_t projection_dim;  /* 512 */
  float   layer_norm_eps;  /* 1e-5 */
  int32_t compute_dtype;   /* PLIPMI_F32 | PLIPMI_BF16 | PLIPMI_F16 */
  int32_t max_batch;       /* images (and captions) per encode call the workspace is sized for */
  int32_t flags;           /* PLIPMI_FLAG_* bits, 0 = the product defaults */
  int32_t graph_batch;     /* small-batch hipGraph replay: 0 = default (batches of <= min(32, max_batch) samples),
                            * > 0 = that many, < 0 = never (plipmi_set_graph_batch changes it later) */
  int32_t text_f16_layers; /* bf16 engine: this many LEADING blocks of the text tower run on IEEE-half (f16) MFMA operands, the
                            * rest of the tower and the whole image tower on bf16.  The bf16 engine's embedding error is mostly
                            * operand rounding in the text tower's first blocks; 0 = a pure bf16 engine,
                            * t_layers = PLIPMI_FLAG_TEXT_TOWER_F16.  The residual stream crosses the switch as the fp32 value the last f16 block's epilogue
                            * computed, re-split for the bf16 blocks (operand plane + 8-bit remainder). */
  int32_t pass_batch;      /* An encode call of B samples runs as ceil(B / pass_batch) back-to-back passes of equal size on the
                            * caller's stream once B >= 2 * pass_batch, so that one pass's per-block activations stay resident in the
                            * 256 MiB Infinity Cache however large the caller's batch is (the reference's `batch_size` is the
                            * caller's, plip.py:31,55).  Same bits either way: a row's embedding does not depend on the batch it
                            * travels in.  0 = automatic (the largest multiple of 32 samples whose per-block working set fits,
                            * 256 for the 16-bit ViT-B/32 engines; no splitting where fewer than 256 samples fit -- the fp32 engine, ViT-L/14 --:
                            * smaller passes lose more in the GEMMs than the cache returns), < 0 = never split. */
} plipmi_config;

/* One pre-LN transformer block, HF CLIPEncoderLayer naming; all DEVICE pointers
 * to fp32, Linear weights stored [out, in] exactly as in the state dict. */
typedef struct plipmi_layer_weights {
  const float *ln1_w, *ln1_b;
  const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;
  const float *ln2_w, *ln2_b;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} plipmi_layer_weights;

/* The whole checkpoint (HF CLIPModel state-dict tensors).  `v_layers` / `t_layers`
 * are HOST arrays of per-layer structs whose members are device pointers.  The
 * engine re-packs everything into its own buffers during plipmi_create, so the
 * caller may free these tensors as soon as the create stream has drained. */
typedef struct plipmi_weights {
  const float* v_class_embedding;   /* [Dv]            vision_model.embeddings.class_embedding */
  const float* v_patch_weight;      /* [Dv,3,P,P]      ...patch_embedding.weight (no bias)      */
  const float* v_pos_embedding;     /* [Np+1,Dv]       ...position_embedding.weight             */
  const float *v_pre_ln_w, *v_pre_ln_b;    /* vision_model.pre_layrnorm */
  const float *v_post_ln_w, *v_post_ln_b;  /* vision_model.post_layernorm */
  const float* visual_projection;   /* [P,Dv]  no bias */
  const plipmi_layer_weights* v_layers;
  const float* t_token_embedding;   /* [V,Dt] */
  const float* t_pos_embedding;     /* [ctx,Dt] */
  const float *t_final_ln_w, *t_final_ln_b;
  const float* text_projection;     /* [P,Dt]  no bias */
  const plipmi_layer_weights* t_layers;
} plipmi_weights;

/* ---- lifetime ----------------------------------------------------------- */
int  plipmi_create(const plipmi_config* cfg, const plipmi_weights* w, void* stream, plipmi_handle* out);
void plipmi_destroy(plipmi_handle h);
/* A second handle on the SAME packed weights with a workspace (activations, staging buffers, captured graphs) of its own: the
 * configuration and the setters' state are copied as they are at the call, the weight memory is shared and lives until the last
 * of the handles that use it is destroyed (any order).  A handle runs one batch per tower at a time -- its workspace is the batch's
 * activations --, so a caller that walks a corpus through ONE tower (the loops of plip.py:41-52 and :64-71, the image side of
 * reproducibility/evaluation/zero_shot/zero_shot.py) gives consecutive batches to two handles on two HIP streams: the launch
 * boundaries, prologues / epilogues and the pooled tail of one batch then run under the GEMMs of the next, as the two towers of a
 * pair do for each other -- configs[3]'s shard 99.1 -> 107.5 k img/s (tools/exp/r06_two_batches.py); same bits per row.  Costs the
 * workspace again (ViT-B/32, max_batch 256: 0.56 GB), no second copy of the weights and no packing time. */
int  plipmi_clone(plipmi_handle src, plipmi_handle* out);
/* The same, with the vision tower at height x width pixels -- HF CLIPModel.get_image_features / forward(...,
 * interpolate_pos_encoding=True) (modeling_clip.py CLIPVisionEmbeddings.interpolate_pos_encoding).  Weights shared and reference-
 * counted as for plipmi_clone (destroy the handles in any order); text tower, heads and setters' state as src's.
 *   grid      : (height / patch_size) x (width / patch_size), floored like HF's strided conv -- pixels past it are ignored.
 *               PLIPMI_ERR_INVALID when a side is under one patch or 1 + grid > 1024 tokens.
 *   positions : the checkpoint's table when the grid has its patch count AND height == width; otherwise the CLS row + the
 *               n0 x n0 patch rows resampled to the grid as torch.nn.functional.interpolate(mode="bicubic", align_corners=False)
 *               does in fp32 (A = -0.75, taps clamped at the border) -- computed once on the GPU during this call.
 *   inputs    : plipmi_encode_image takes fp32 [B,3,height,width], plipmi_encode_image_u8 uint8 [B,height,width,3].
 *   max_batch : 0 = the largest B with B * (1 + grid) <= src's max_batch * src's vision tokens (>= 1): about src's workspace;
 *               > 0 as given.  Both towers' calls take at most that many samples on the new handle.
 * pass_batch, the graph staging, the attention kernels and the fused-kernel choices follow the new token count (197 tokens at
 * 448 x 448 for ViT-B/32: the streamed MFMA attention; 65 .. 80: the fused q/k/v + attention kernel).  plipmi_clone of the new
 * handle keeps its size and table. */
/* (Additive: the version number and every existing entry are unchanged; a caller probes for the symbol.) */
int  plipmi_clone_resolution(plipmi_handle src, int height, int width, int max_batch, plipmi_handle* out);
int  plipmi_version(void);
const char* plipmi_last_error(void);
/* name of the device the engine runs on ("gfx950:..."), for logs */
const char* plipmi_device_name(plipmi_handle h);

/* ---- the hot path ----------------------------------------------------------
 * pixels  : fp32 [B,3,H,W] NCHW (H = W = image_size, or the handle's plipmi_clone_resolution size), already CLIP-normalised (what CLIPProcessor /
 *           reproducibility/embedders/transform.py:45-52 produce)
 * out     : fp32 [B, projection_dim]; un-normalised when normalize == 0 (what
 *           PLIP.encode_images returns, plip.py:53), L2-normalised rows when 1
 *           (what CLIPEmbedder returns, embedders/plip.py:53).
 * B may be anything in [0, max_batch]. */
int plipmi_encode_image(plipmi_handle h, const float* pixels, int B, float* out, int normalize, void* stream);

/* Same, from raw tiles: uint8 [B,H,W,3] (HWC RGB, already image_size x image_size -- or the handle's size, plipmi_clone_resolution).  The CLIP normalisation
 * (u8/255 - mean)/std of reproducibility/embedders/transform.py:45-52 / HF CLIPImageProcessor is fused into the
 * patch GEMM's operand load (large batches: im2col on load from the HWC bytes, one fma per pixel; small ones: a fused unfold pass --
 * the same bits), so a tile crosses PCIe and HBM as 150 KB instead of 602 KB of fp32. */
int plipmi_encode_image_u8(plipmi_handle h, const uint8_t* tiles, int B, float* out, int normalize, void* stream);

/* ids            : int64 [B, context_length] token ids
 * attention_mask : int64 [B, context_length] (1 = token, 0 = padding) or NULL;
 *                  combined with the causal mask like HF create_causal_mask
 * eos_token_id   : pooled row = first position whose id == eos_token_id (0 if
 *                  none); eos_token_id < 0 or == 2 selects "first arg-max of the
 *                  ids" (legacy HF configs and OpenAI-clip), modeling_clip.py:561-581 */
int plipmi_encode_text(plipmi_handle h, const int64_t* ids, const int64_t* attention_mask, int B,
                       int eos_token_id, float* out, int normalize, void* stream);

/* Token ids outside [0, vocab_size).  The reference's embedding lookup raises on them (plip.py:68 -> nn.Embedding; on a
 * GPU as a device-side assert that surfaces at the next synchronisation).  plipmi_encode_text only enqueues work, so the
 * ids -- device memory -- are checked BY the embedding kernel: it clamps the lookup (no wild read) and raises a flag in
 * host-visible memory.  The flag is reported, once, as PLIPMI_ERR_TOKEN_ID (= the embeddings of an earlier encode_text
 * are invalid) by this function -- call it after synchronising the stream -- and by the next plipmi_encode_text on the
 * handle, which then enqueues nothing: a caller that feeds a long id matrix in chunks may therefore see the error from a
 * LATER chunk's call, with the earlier chunks' (valid and invalid) rows already written.  The image-side entry points and
 * the heads never report it: a bad caption does not fail an unrelated plipmi_encode_image. */
int plipmi_check_async(plipmi_handle h);

/* Small-batch launch amortisation.  An encode call of at most `max_batch` samples (default min(32, cfg.max_batch), see
 * plipmi_config.graph_batch; 0 = never) replays a captured hipGraph of its ~170 kernel launches instead of issuing
 * them one by one: the first call of a shape (tower, batch, normalise, pooling rule, mask present) runs eagerly, the
 * second captures on the caller's stream, later ones replay.  Inputs / outputs of a replay travel through handle-owned
 * staging buffers (two device-to-device copies per call), results are bit-identical to the eager path.  The reference's
 * zero_shot_classification runs both towers at batch 8 (plip.py:90-91), where the step is launch-bound. */
int plipmi_set_graph_batch(plipmi_handle h, int max_batch);
/* plipmi_config.pass_batch as the handle resolved it (0 = encode calls are never split): a host layer that drives BOTH towers of a
 * batch on two streams (plip_amd.Engine.encode_pair) cuts the batch itself, so that the towers of one pass finish together before
 * the next pass starts -- the rhythm of back-to-back calls of pass_batch samples, which is what the split is meant to reproduce. */
int plipmi_get_pass_batch(plipmi_handle h);
/* Do two HIP streams run their kernels SIDE BY SIDE?  HIP maps streams onto a few hardware queues, and which queue a new stream
 * lands on depends on how many streams the process created before; two streams on one queue execute in order however independent
 * their work is -- a caller that puts the two towers of a pair on such streams gets the one-stream step.  Runs a
 * workgroup that only waits (no memory traffic) for 250 us on each stream at once, three times, and writes
 * *ratio = shortest elapsed time / 250 us: about 1.0-1.2 when the streams overlap, about 2 when they share a queue.  Synchronises
 * both streams; not for use under stream capture.  plip_amd.Engine.encode_pair picks its second stream with it, once. */
int plipmi_streams_overlap(plipmi_handle h, void* stream_a, void* stream_b, float* ratio);

/* Latency path (16-bit engines; OFF by default).  The big GEMM tiles walk K serially whatever M is -- fc2 at batch 8 is 48
 * dependent K tiles for 24 workgroups -- so after plipmi_set_latency_batch(h, n) an encode call of at most n samples runs every
 * GEMM of its tower on the split-K small-M kernel instead (csrc/gemm_skinny.hip): pair latency 1.16 -> 0.79 ms at batch 1,
 * 1.32 -> 1.09 ms at batch 8 (it loses from batch 16 on).  Same arithmetic, another fp32 summation order -- which moves the
 * roundings of the 16-bit activations: embeddings of the two regimes differ by up to 6e-4 (both inside the parity bar).
 * INSIDE a regime a row's embedding does not depend on the batch it arrives in, bit for bit; with the path off (n = 0, the
 * default) that holds for every batch size. */
int plipmi_set_latency_batch(plipmi_handle h, int max_batch);

/* Caption packing (16-bit engines, off by default; PLIPMI_FLAG_PACK_CAPTIONS starts with it on).  CLIPTextTransformer is causal and
 * pools the EOS row only (modeling_clip.py:543-581), so the positions behind a caption's EOS token -- the tokenizer's
 * padding to 77 -- cannot influence text_embeds; the reference computes them anyway.  With packing on, plipmi_encode_text
 * lays the captions' live rows (0 .. EOS) end to end and runs every kernel of the text tower on those rows only: lengths,
 * row offsets and the live-row count are derived from `ids` ON THE DEVICE (no host synchronisation; the path stays
 * graph-capturable), the GEMMs size their grids for the padded worst case and retire dead tiles at once, attention takes
 * per-caption lengths.  text_embeds are BIT-IDENTICAL to the padded computation.  A caption of L tokens then costs L/77 of
 * a padded one.  The default (off) executes every padded position, which is what the bench's headline line measures.
 * A text tower whose head_dim is not 64 has no packed form: PLIPMI_ERR_INVALID (here and for PLIPMI_FLAG_PACK_CAPTIONS). */
int plipmi_set_text_packing(plipmi_handle h, int on);

/* Per-token tower outputs -- what HF CLIPModel.vision_model / .text_model return with output_hidden_states /
 * output_attentions (modeling_clip.py CLIPVisionTransformer, CLIPTextTransformer, eager attention).
 * plipmi_tower_shape: shape[4] = {S tokens, D width, H heads, L blocks} of `tower` on this handle (S of the vision tower
 * follows the handle's image size: plipmi_clone_resolution).  plipmi_encode_tower_outputs, for B <= max_batch samples:
 *   input          : vision fp32 pixels [B,3,H,W] as plipmi_encode_image; text int64 ids [B, context_length]
 *   attention_mask : text only, as plipmi_encode_text (honoured by the attention and the probabilities); NULL for vision
 *   eos_token_id   : text pooling rule, as plipmi_encode_text
 *   last_hidden    : fp32 [B,S,D]  vision: the encoder output; text: final_layer_norm(encoder output)
 *   pooled         : fp32 [B,D]    vision: post_layernorm(CLS row); text: final_layer_norm of the EOS row
 *   hidden_states  : fp32 [L+1,B,S,D]  [0] = the embeddings (vision: after pre_layrnorm), [l] = the output of block l-1
 *   attentions     : fp32 [L,B,H,S,S]  softmax probabilities; masked entries exactly 0, every row with a live key sums to 1
 * Any output may be NULL, not all of them.  Runs eagerly (no graph), every block on every token, the text tower on unpacked rows
 * through the q/k/v GEMM + attention pair; none of the handle's settings change, and the encode entries return the same bits
 * after it as before.  Blocks, hidden states and pooled rows are those of the PLIPMI_FLAG_DENSE_LAST_BLOCK forward. */
int plipmi_tower_shape(plipmi_handle h, int tower, int32_t* shape);
int plipmi_encode_tower_outputs(plipmi_handle h, int tower, const void* input, const int64_t* attention_mask, int B, int eos_token_id,
                                float* last_hidden, float* pooled, float* hidden_states, float* attentions, void* stream);

/* Attention summaries -- what the attention probabilities are mostly pulled for, without the [L,B,H,S,S] tensor.  For a tower of L
 * blocks, H heads and S tokens let P_l[b,h] be block l's S x S probabilities exactly as plipmi_encode_tower_outputs defines them (HF
 * eager attention, the text tower under causal + padding mask, masked entries exactly 0, a row with no live key all zeros), and r_b
 * the pooled row of sample b: row 0 (CLS) for vision, the row the eos_token_id rule of plipmi_encode_text picks for text.
 *   pooled_attention : fp32 [L,B,H,S]  P_l[b,h][r_b, :] -- which tokens the pooled token looked at, the bits `attentions` holds there
 *   rollout_matrix   : fp32 [B,S,S]    R_L[b], with R_0 = I and R_l = (1/2 A_l + 1/2 I) R_{l-1}, A_l = (1/H) sum_h P_l[b,h] summed in
 *                                      the order h = 0 .. H-1, the product summed over k = 0 .. S-1, all in fp32: attention rollout
 *                                      (Abnar & Zuidema 2020) with residual weight 1/2 and head mean.  A dead row i of A_l leaves
 *                                      1/2 e_i: defined, not an error.  Rows with live keys throughout sum to 1.
 *   rollout          : fp32 [B,S]      row r_b of R_L[b]
 * input, attention_mask, eos_token_id and the B <= max_batch rule are those of plipmi_encode_tower_outputs.  Any output may be NULL,
 * not all of them.  The walk is plipmi_encode_tower_outputs' (eager, every block dense on every token, q/k/v GEMM + attention as two
 * kernels) with the summary kernels reading each block's qkv activation; the rollout ping-pongs between two [B,S,S] buffers in handle
 * scratch outside the tower workspace, reserved on first use and freed by plipmi_destroy (a non-NULL rollout_matrix serves as one of
 * them) -- 2.7 MB per image for ViT-L/14@336 against 511 MB of attentions.  None of the handle's settings change, and the encode
 * entries return the same bits after it as before. */
int plipmi_encode_attention_summary(plipmi_handle h, int tower, const void* input, const int64_t* attention_mask, int B, int eos_token_id,
                                    float* pooled_attention, float* rollout, float* rollout_matrix, void* stream);

/* Dense image-text similarity -- one score per token (CLS + every patch) and text prompt: "where in this tile is <prompt>?".
 * With X [B*S, Dv] the vision encoder's output for B <= max_batch images (pixels fp32 [B,3,H,W] at the handle's size, as
 * plipmi_encode_image; handles of plipmi_clone_resolution included) let
 *   E = post_layernorm(X) . visual_projection^T   on EVERY row, [B,S,P], computed in fp32 on every engine dtype (LayerNorm in fp32,
 *       the projection on the exact-fp32 MFMA GEMM against the fp32 weights the pooled head uses).
 *   token_embeds : fp32 [B,S,P], optional (may be NULL): E, un-normalised -- HF visual_projection(vision_model.post_layernorm(
 *                  vision_model(pixel_values).last_hidden_state))
 *   similarity   : fp32 [B,S,C], optional (may be NULL): similarity[b,s,c] = scale * <E[b,s] / |E[b,s]|, t_c / |t_c|>.  Row s = 0 is the
 *                  CLS token: what logits_per_image holds for the image (at scale = exp(logit_scale)).  softmax != 0: the softmax over c
 *                  of those values, max-subtracted.
 *   text_embeds  : fp32 [C,P] on the device, 16-byte aligned, 1 <= C <= PLIPMI_TOKEN_SIM_MAX_C; the rows need not be normalised.  No
 *                  epsilon anywhere: a zero row (of E or of text_embeds) gives non-finite scores, as with plipmi_l2_normalize.
 * The walk is plipmi_encode_tower_outputs' for the vision tower: eager, every block dense on every token.  Behind it run a LayerNorm
 * over all B*S rows, the projection GEMM and ONE kernel (csrc/token_scores.hip) that forms |E|^2, the C dot products, both
 * normalisations, the scale and the softmax per row with fixed-order sums: a row's bits depend on neither B nor its place in the batch.
 * The text rows are normalised inside that kernel, in LDS; the LayerNorm'd rows and -- when token_embeds is NULL -- E live in handle
 * scratch outside the tower workspace, reserved on first use and freed by plipmi_destroy (clones and resolution handles own theirs).
 * No handle setting is written, and the encode entries return the same bits after the call as before.
 * PLIPMI_ERR_INVALID, with a message that names the argument, before any launch: a null handle (checked first), null pixels or
 * text_embeds, both outputs NULL, C outside 1 .. PLIPMI_TOKEN_SIM_MAX_C, B > max_batch, a projection_dim that is no multiple of 32.
 * B == 0 is PLIPMI_OK and launches nothing. */
#define PLIPMI_TOKEN_SIM_MAX_C 64
int plipmi_encode_token_similarity(plipmi_handle h, const float* pixels, int B, const float* text_embeds, int C,
                                   float scale, int softmax, float* token_embeds, float* similarity, void* stream);

/* in-place row-wise x / sqrt(sum x^2), no epsilon (modeling_clip.py:57-65) */
int plipmi_l2_normalize(plipmi_handle h, float* x, int N, int D, void* stream);

/* logits_per_image[i,j] = scale * <img_i, txt_j>  ([Ni,Nt], required)
 * logits_per_text       = its transpose            ([Nt,Ni], optional, may be NULL)
 * argmax_per_image[i]   = first arg-max_j          (int32 [Ni], optional, may be NULL)
 * img [Ni,D], txt [Nt,D] fp32; pass scale = exp(logit_scale) for CLIPModel.forward,
 * 1.0 for the plain dot product of the zero-shot / retrieval heads. */
int plipmi_logits(plipmi_handle h, const float* img, int Ni, const float* txt, int Nt, int D, float scale,
                  float* logits_per_image, float* logits_per_text, int32_t* argmax_per_image, void* stream);

/* top-k columns of each row of scores [N,M], descending (ties: lower index first);
 * idx int64 [N,k].  Replaces argsort()[:, -k:][:, ::-1] (plip.py:84). */
int plipmi_topk(plipmi_handle h, const float* scores, int N, int M, int k, int64_t* idx, void* stream);

/* Resize (Pillow-exact 8-bit bicubic) + centre crop on the GPU, the step in front of plipmi_encode_image_u8:
 * replaces the host-side `_transform` Resize/CenterCrop (reproducibility/embedders/transform.py:45-48) and the
 * CLIPImageProcessor resize + center_crop behind `self.preprocess(images=...)` (plip.py:32-35) for batches of
 * equally sized uint8 HWC images.  src [B,H,W,3] -> dst [B,n_px,n_px,3], bit-identical to
 * Image.resize((nw,nh), BICUBIC).crop(...).  The caller supplies Pillow's fixed-point tables restricted to the crop
 * window (plip_amd/preprocess.py:resize_crop_plan): x/ybounds int32 [n_px,2] = (first input index, taps),
 * x/ycoef int32 [n_px,ksize]; a NULL pair means that axis already has the right size (crop only, at left/top).
 * tmp [B,nrows,n_px,3] holds source rows row0..row0+nrows after the horizontal pass. */
int plipmi_resize_crop_u8(plipmi_handle h, const uint8_t* src, int B, int H, int W, int n_px, const int32_t* xbounds,
                          const int32_t* xcoef, int xksize, int left, const int32_t* ybounds, const int32_t* ycoef,
                          int yksize, int top, int row0, int nrows, uint8_t* tmp, uint8_t* dst, void* stream);

/* The same resize + centre crop for a RAGGED batch: B uint8 RGB images, each with its own height and width, packed in one
 * device buffer -- image b is hw[b] = {height, width} rows of width * 3 bytes at src + offsets[b].  dst [B,n_px,n_px,3] is
 * bit-identical, image by image, to Image.resize((nw,nh), BICUBIC).crop(...) with the geometry of plipmi_resize_crop_u8's caller
 * (shortest edge -> n_px, long edge int(n_px * long / short), crop_rule 0 = torchvision CenterCrop, 1 = HF center_crop).  Nothing
 * per size is built on the host: Pillow's coefficient tables (float64, unfused) are computed on the device, in `workspace`.
 *   offsets int64 [B], hw int32 [B,2]   device buffers;  offsets_host, hw_host: host copies of the same values, read during the
 *                                        call only -- every check below and the sizing of the intermediate use them
 *   ksize      taps the coefficient rows hold: at least 2 * ceil(2 * max(s, 1)) + 1 for the largest in / out ratio s of any axis
 *              of the batch
 *   workspace  device scratch of at least the workspace function's bytes for the same (hw_host, B, n_px, ksize), caller-owned (tables
 *              + the horizontally filtered rows); nothing is allocated here and nothing synchronises: four kernel launches
 * PLIPMI_ERR_INVALID before any launch: a side < 1, an in / out ratio above 64, offsets[b] + height * width * 3 > src_bytes,
 * B > 65535, ksize or workspace_bytes too small.  B = 0 launches nothing. */
int plipmi_resize_crop_u8_ragged(plipmi_handle h, const uint8_t* src, size_t src_bytes, const int64_t* offsets, const int32_t* hw,
                                 const int64_t* offsets_host, const int32_t* hw_host, int B, int n_px, int crop_rule, int ksize,
                                 void* workspace, size_t workspace_bytes, uint8_t* dst, void* stream);
/* bytes of `workspace` for that call (0 for a bad argument); host arithmetic only */
size_t plipmi_resize_ragged_workspace(const int32_t* hw_host, int B, int n_px, int ksize);

/* ---- slide regions ---------------------------------------------------------
 * (Additive: the version number and every existing entry are unchanged; a caller probes for the symbols.)
 * A slide region on the device -- uint8 RGB, H rows of W pixels, row y at region + y * pitch_bytes (pitch_bytes >= 3 W: a view of a
 * larger array works as it is; rows may start at any byte) -- cut into a grid of tile x tile windows, tile (i, j) with its top-left
 * pixel at (y0 + i * stride, x0 + j * stride), flat index i * cols + j.  stride < tile overlaps, stride > tile leaves gaps.  The
 * caller states rows and cols; every tile must lie inside the region (rows = (H - y0 - tile) / stride + 1 is the most that fit).
 *
 * plipmi_region_select: counts[i * cols + j] = the tile's pixels that are tissue, by integer arithmetic only (the same numbers on every
 * platform; numpy restatement: plip_amd/preprocess.py tissue_mask).  With mx / mn the largest / smallest of r, g, b and
 * luma = (77 r + 150 g + 29 b + 128) >> 8, a pixel is tissue iff 255 (mx - mn) >= sat_min * mx and luma_min <= luma <= luma_max
 * (each threshold 0 .. 255).  kept[0 .. K) = the flat indices of the tiles with counts >= min_count, ascending; *n_kept = K; the rest
 * of kept is not written.  counts, kept int32 [rows * cols], n_kept int32 [1], all on the device.  Two launches, no allocation, no
 * synchronisation.  rows * cols == 0 launches nothing and sets *n_kept = 0.
 *
 * plipmi_region_gather: dst[b] = tile kept[first + b] for b in 0 .. B, dst uint8 [B, tile, tile, 3] contiguous -- the batch the u8
 * encode entry (tile = the engine's image size) or plipmi_resize_crop_u8 takes.  kept is device memory (plipmi_region_select's, or any
 * int32 list of flat indices); first + B <= rows * cols with rows the most that fit.  An index outside the grid is clamped to it on
 * the device: wrong pixels, never an address outside the region.  One launch; B == 0 launches nothing.
 *
 * Both return PLIPMI_ERR_INVALID with a message before any launch: a null pointer, a tile outside the H x W region, pitch_bytes < 3 W,
 * a region of 4 GiB or more (H * pitch_bytes; pass it in bands), a threshold outside 0 .. 255, a negative min_count / first / B. */
int plipmi_region_select(plipmi_handle h, const uint8_t* region, int H, int W, int64_t pitch_bytes, int y0, int x0, int tile, int stride,
                         int rows, int cols, int sat_min, int luma_min, int luma_max, int min_count, int32_t* counts, int32_t* kept,
                         int32_t* n_kept, void* stream);
int plipmi_region_gather(plipmi_handle h, const uint8_t* region, int H, int W, int64_t pitch_bytes, int y0, int x0, int tile, int stride,
                         int cols, const int32_t* kept, int first, int B, uint8_t* dst, void* stream);

/* ---- augmented views --------------------------------------------------------
 * (Additive: the version number and every existing entry are unchanged; a caller probes for the symbol.)
 * plipmi_warp_u8: dst[b] (uint8 [B, out_h, out_w, 3] contiguous) = source image b warped by coefficient row b, with the bytes of
 * Pillow's Image.transform((out_w, out_h), AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor=...) -- the call torchvision's
 * RandomAffine / RandomPerspective / F.affine / F.perspective make on a PIL image (reproducibility/embedders/transform.py
 * _train_transform).  Source image b is uint8 RGB, H rows of W pixels, row y at src + b * image_stride_bytes + y * pitch_bytes
 * (pitch_bytes >= 3 W; rows and images may start at any byte); image_stride_bytes == 0: all B outputs sample the ONE image at src (V
 * views of a tile, its eight dihedral views).  coeffs double [B,8] ON THE DEVICE: the output -> input map of output pixel (x, y), in
 * fp64 with every product and sum rounded once in the order written (numpy restatement: plip_amd/preprocess.py warp_reference):
 *     xin = x + 0.5, yin = y + 0.5
 *     perspective == 0:  xs = (a0 xin + a1 yin) + a2,  ys = (a3 xin + a4 yin) + a5                   (a6, a7 are not read)
 *     perspective == 1:  the same two, each divided by den = (a6 xin + a7 yin) + 1
 * windows int32 [B,5] on the device, or NULL: (wy, wx, wh, ww, flip) -- the image that is sampled is rows wy .. wy + wh, columns wx ..
 * wx + ww of the source, mirrored left-right when flip != 0 (crop, flip and warp in one pass, bytes equal to doing them in turn);
 * NULL = the whole source, not mirrored.  A point with 0 <= xs < ww and 0 <= ys < wh is sampled bilinearly at (xs - 0.5, ys - 0.5)
 * with the columns and the first row clipped to the window and the result truncated to a byte; every other point (NaN included) gets
 * fill_rgb = r | g << 8 | b << 16.
 * Read on the device and REFUSED there, not clamped: a window that does not lie inside the H x W source (wy, wx < 0, wh, ww < 1, wy +
 * wh > H, wx + ww > W), and with perspective == 1 a row whose den is not > 0 at the four corners (0, 0), (out_w, 0), (0, out_h),
 * (out_w, out_h) of the output (den is linear, so it is then > 0 at every pixel; Pillow leaves a vanishing den undefined).  Such an
 * image comes out all fill and no address outside the source is formed; the call still returns PLIPMI_OK.  The entry cannot read
 * the rows without synchronising, so it does not: callers that hold them on the host refuse such rows by name before they are uploaded (plip_amd/preprocess.py
 * check_perspective, plip_amd/augment.py).
 * One launch, no allocation, no synchronisation; B == 0 launches nothing.  PLIPMI_ERR_INVALID with a message before any launch: a
 * null handle / src / coeffs / dst, B < 0, a side < 1, pitch_bytes < 3 W, image_stride_bytes < 0, a source image (H * pitch_bytes) or
 * an output image (3 out_h out_w) of 2 GiB or more (the kernel's offsets inside one image are 32-bit), perspective other than 0 / 1,
 * bits of fill_rgb above the third byte, coeffs not 8-byte / windows not 4-byte aligned. */
int plipmi_warp_u8(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes,
                   const int32_t* windows, const double* coeffs, int perspective, int out_h, int out_w, uint32_t fill_rgb, uint8_t* dst,
                   void* stream);

/* Fused similarity + top-k: for every row q of keys [Nq,D] the k rows j of space [Ns,D] with the largest <q, space_j>,
 * descending (ties: lower j first), WITHOUT materialising the [Nq,Ns] score matrix: scores are produced in
 * [<=4096, <=8192] fp32 panels (MFMA fp32 GEMM) and folded into per-row running lists.  idx int64 [Nq,k] (required),
 * vals fp32 [Nq,k] (optional, may be NULL).  1 <= k <= min(Ns, 1024), D % 32 == 0.  Scratch (<= ~150 MiB) is
 * allocated inside the handle on first use.  Replaces the per-query `t.dot(image_embeddings.T).argsort()[-50:][::-1]`
 * loop of reproducibility/evaluation/retrieval/retrieval.py:13-18 and cosine_sim.argsort()[:, -k:][:, ::-1] of
 * plip.py:78-87 for corpora whose [N,N] matrix would not fit. */
int plipmi_similarity_topk(plipmi_handle h, const float* keys, int Nq, const float* space, int Ns, int D, int k,
                           int64_t* idx, float* vals, void* stream);

/* ---- linear-probe head ---------------------------------------------------------
 * The reference's third evaluation head (linear_classifier.py): K one-vs-rest logistic problems on cached embeddings,
 *   f_k(w, b) = (1/N) sum_i c_ik log(1 + exp(-t_ik (x_i.w + b))) + alpha/2 |w|^2,   t_ik = +1 if y_i is problem k's label else -1,
 * the objective of scikit-learn's SGDClassifier(loss="log_loss", penalty="l2", alpha); the intercept is not regularised.
 *   X      fp32 [N, D] device, 16-byte aligned, D % 4 == 0, 4 <= D <= 1024
 *   y      int32 [N] device, class indices.  K >= 2: problem k's positive label is k.  K == 1 is the two-class problem: positive
 *          label 1.  A label that is no problem's positive one is a negative everywhere (the host checks the range).
 *   pos_w, neg_w  fp32 [K] device: c_ik for the positives / negatives of problem k (class_weight="balanced": N / (C count_k) and 1;
 *          two classes: the two class weights)
 *   WB     fp32 [K, D + 1] device: row k = w_k, then b_k.  1 <= K <= PLIPMI_PROBE_MAX_K.
 * plipmi_probe_fit minimises every f_k from the point in WB_inout (zeros = scikit-learn's start) and leaves the result there:
 * L-BFGS (10 pairs) per problem with a backtracking line search on the host, one fused loss-and-gradient pass over X per
 * evaluation for all K trial points (csrc/probe.hip: fp32 MFMA, X read once per pass, fixed-order reductions -- the same inputs
 * give the same bits).  Unlike every other entry it SYNCHRONISES the stream (once per evaluation).  A problem stops when
 * the infinity norm of its gradient is <= gtol; PLIPMI_ERR_NOT_CONVERGED when one has not got there after max_iter iterations --
 * WB_inout and info_out then hold the best point found.  This is a converged, deterministic solver of the reference's objective,
 * not its early-stopped sequential SGD: there is no seed.  Scratch lives on the handle (freed by plipmi_destroy), outside the
 * tower workspace.
 * plipmi_probe_predict: decision fp32 [N, K] = X W^T + b (optional, may be NULL) and pred int32 [N] = the first arg-max over
 * the K problems; K == 1: 1 if the decision value is > 0 else 0.  Enqueues only. */
#define PLIPMI_PROBE_MAX_K 64
typedef struct plipmi_probe_info {
  int32_t iterations;    /* accepted L-BFGS steps of the problem that took most */
  int32_t evaluations;   /* loss-and-gradient passes over X */
  int32_t converged;     /* problems that met gtol (== K on PLIPMI_OK) */
  int32_t reserved;
  double  grad_norm;     /* max over the problems of |grad f_k|_inf at the returned point */
  double  loss[PLIPMI_PROBE_MAX_K];  /* f_k at the returned point */
} plipmi_probe_info;
int plipmi_probe_fit(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int K, const float* pos_w, const float* neg_w,
                     float alpha, int max_iter, float gtol, float* WB_inout, plipmi_probe_info* info_out, void* stream);
int plipmi_probe_predict(plipmi_handle h, const float* X, int N, int D, const float* WB, int K, float* decision, int32_t* pred,
                         void* stream);

/* ---- softmax (multinomial) linear probe ----------------------------------------
 * (Additive, like the entries above it: the version number and every existing entry are unchanged; a caller probes for the symbol.)
 * The other linear-probe objective, ONE softmax over all classes -- the CLIP paper's protocol, scikit-learn's
 * LogisticRegression(C, max_iter=1000) (multinomial, L-BFGS), and the reference's own fine-tuning head (LinearClassifier +
 * nn.CrossEntropyLoss(), reproducibility/fine_tuning/finetune.py) with the tower frozen:
 *   f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k(x_i.w_k + b_k) - (x_i.w_{y_i} + b_{y_i})) + alpha/2 |W|_F^2
 * for C >= 2 classes, always C rows (no special two-class shape); the intercepts are not regularised; alpha = 1 / (C_sklearn N).
 *   X, y     as plipmi_probe_fit.  A label outside [0, C) gives its row weight 0 (the host checks the range).
 *   class_w  fp32 [C] device: cw (class_weight="balanced": N / (C count_k)), or NULL = all ones
 *   WB       fp32 [C, D + 1] device: row k = w_k, then b_k.  2 <= C <= PLIPMI_PROBE_MAX_K.
 * Three or more classes: the minimiser is LogisticRegression(C = 1 / (alpha N), class_weight)'s.  f does not change when a constant
 * is added to every intercept; the gradient with respect to b sums to zero, so a fit from zeros stays on sum(b) = 0 up to rounding
 * (compare b - mean(b)), and the columns of the optimal W sum to zero.  Two classes: W[1] - W[0] and b[1] - b[0] are
 * LogisticRegression(C = 2 / (alpha N))'s binary coef_ and intercept_ (the two-row softmax is the binary problem at HALF the penalty).
 * plipmi_softmax_fit minimises f from the point in WB_inout and leaves the result there: one L-BFGS (10 pairs, backtracking line
 * search, on the host) over all C (D + 1) variables, one loss-and-gradient evaluation per trial point (csrc/probe_softmax.hip: fp32
 * MFMA, X read once per evaluation for C <= 16 and 1 + ceil(C / 16) times beyond, fixed-order reductions -- the same inputs give the
 * same bits).  Like plipmi_probe_fit it SYNCHRONISES the stream once per evaluation, stops when |grad f|_inf <= gtol, and returns
 * PLIPMI_ERR_NOT_CONVERGED with the best point found after max_iter iterations.  info_out (may be NULL) keeps its layout: loss[0] = f,
 * converged is 0 or 1.  Scratch is the handle's probe scratch.  Predictions and decision values: plipmi_probe_predict on WB, K = C. */
int plipmi_softmax_fit(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int C, const float* class_w, float alpha,
                       int max_iter, float gtol, float* WB_inout, plipmi_probe_info* info_out, void* stream);

/* ---- k-means on cached embeddings ----------------------------------------------
 * (Additive, like the entries above it: the version number and every existing entry are unchanged; a caller probes for the symbols.)
 * Lloyd's algorithm over X fp32 [N, D] (device, 16-byte aligned, D % 4 == 0, 4 <= D <= 1024, finite values) with
 * 1 <= K <= min(N, PLIPMI_KMEANS_MAX_K) centres fp32 [K, D] (16-byte aligned too).  Both metrics are one score with a per-centre bias,
 *   s_ik = x_i . c_k + h_k,      label_i = the FIRST arg-max over k (ties go to the lower k):
 *   PLIPMI_KMEANS_EUCLIDEAN  h_k = -1/2 |c_k|^2, d_i = max(0, |x_i|^2 - 2 s_i), new centre = the mean of its members
 *                            (scikit-learn's KMeans(algorithm="lloyd"))
 *   PLIPMI_KMEANS_COSINE     spherical k-means: rows are used as given (the caller passes unit rows), h_k = 0, d_i = max(0, 1 - s_i),
 *                            new centre = the members' sum divided by its norm; a zero sum counts as an empty cluster
 * inertia = sum_i d_i.  csrc/kmeans.hip: the scores are exact-fp32 MFMA products, no N x K buffer exists, every floating-point
 * reduction has a fixed order and there are no floating-point atomics -- the same inputs give the same bits on every run.
 * Whatever the input, a label written is in [0, K).  Scratch is a workspace of the handle's own, grown on first use.
 * Anything outside the limits above (a null pointer, an unknown metric, D % 4, D outside 4 .. 1024, K outside 1 .. min(N, 4096), a
 * misaligned X) is PLIPMI_ERR_INVALID with a message that names the limit, before any launch.
 *
 * plipmi_kmeans_seed: plain k-means++ D^2 sampling (NOT scikit-learn's greedy variant), entirely on the device, no synchronisation,
 * from K uniforms in [0, 1) on the HOST.  Pick 0 is row floor(u_0 N).  Step t: mind_i is lowered to the distance d to the centre
 * just picked, mind is summed in float64 in a fixed order, and the pick is the first row whose float64 prefix sum over ascending i
 * exceeds u_t * total (total == 0: the lowest row not yet picked).  centers[t] = X[picks[t]] bit for bit; picks (device int32 [K])
 * may be NULL.
 * plipmi_kmeans_assign: labels int32 [N] and scores fp32 [N] (s_i,label; may be NULL) for the given centres.  Enqueues only.
 * plipmi_kmeans_fit: Lloyd's loop on the host from centers_inout, which it overwrites.  It SYNCHRONISES the stream once per
 * iteration (like plipmi_probe_fit) and reads back a few bytes: the number of changed labels, the number of empty clusters and the
 * centre shift sum_k |delta c_k|^2.  It stops when no label changed or when the shift is <= tol_abs (info.converged = 1), or after
 * max_iter iterations (converged = 0, still PLIPMI_OK: reaching max_iter is normal for k-means).  Empty clusters: in ascending k,
 * an empty cluster takes as its centre the row with the largest d_i not yet taken in this iteration (ties: the lower row); each move
 * counts in info.relocations, and an iteration that moved a centre does not stop the loop (the rare path: it copies the scores to
 * the host and synchronises once more).  The shift counts the clusters that have members.  On return labels, scores, counts [K],
 * reps [K] (the member with the largest score, ties to the lower row; scores / counts / reps may be NULL) and info.inertia all
 * belong to the returned centres. */
#define PLIPMI_KMEANS_MAX_K 4096
enum { PLIPMI_KMEANS_EUCLIDEAN = 0, PLIPMI_KMEANS_COSINE = 1 };
typedef struct plipmi_kmeans_info {
  int32_t iterations;    /* Lloyd iterations run (scikit-learn's n_iter_) */
  int32_t converged;     /* 1: no label changed, or the shift fell to tol_abs; 0: stopped at max_iter */
  int32_t relocations;   /* empty clusters given a new centre, over the whole fit */
  int32_t reserved;
  double  inertia;       /* sum_i d_i at the returned centres */
  double  center_shift;  /* sum_k |delta c_k|^2 of the last iteration */
} plipmi_kmeans_info;
int plipmi_kmeans_seed(plipmi_handle h, const float* X, int N, int D, int K, int metric, const double* u_host, float* centers,
                       int32_t* picks, void* stream);
int plipmi_kmeans_assign(plipmi_handle h, const float* X, int N, int D, const float* centers, int K, int metric, int32_t* labels,
                         float* scores, void* stream);
int plipmi_kmeans_fit(plipmi_handle h, const float* X, int N, int D, int K, int metric, int max_iter, double tol_abs,
                      float* centers_inout, int32_t* labels, float* scores, int32_t* counts, int32_t* reps, plipmi_kmeans_info* info,
                      void* stream);

/* ---- stain normalisation -----------------------------------------------------
 * (Additive, like the entries above it: the version number and every existing entry are unchanged; a caller probes for the symbols.)
 * Macenko's method on uint8 RGB images, the project's own definition (plip_amd/preprocess.py stain_fit_reference /
 * stain_apply_reference is its float64 numpy statement; csrc/stain.hip).  Sources are strided like plipmi_warp_u8's: B images of
 * H x W pixels, rows pitch_bytes >= 3 W apart, images image_stride_bytes apart, rows and images starting at any byte, one image below
 * 2 GiB.  lut_dev: double [256] on the device, lut[v] = -log((v + 1) / Io), built by the CALLER (numpy) so that a pixel's optical
 * density is the oracle's bit for bit; the device takes no logarithm.  All arithmetic is fp64 without contraction; every
 * floating-point sum has a fixed order, the only atomics are integer: the same input gives the same bits on every run.
 *
 * plipmi_stain_fit: fits over the SAMPLED pixels (y % step == 0 and x % step == 0) of each image, or with pooled != 0 ONE fit over
 * those of all B images (image, row, column order).  A pixel is tissue when no channel's density is below beta; mean and sample
 * covariance of the n tissue densities; its two principal eigenvectors by cyclic Jacobi, each negated when its components sum below
 * zero; the angle atan2 of every tissue pixel in that plane as a float32 key; the alpha-th and (100 - alpha)-th percentile of the keys
 * (numpy's default linear method, the order statistics selected EXACTLY by a radix select, interpolated in fp64); the two stain
 * vectors, haematoxylin (the larger first component) first, HE [3,2]; P = (HE^T HE)^-1 HE^T [2,3]; maxC[j] = the 99th percentile of the
 * float32 keys (P . OD)[j] over EVERY sampled pixel.  fits_out: double [F, 16] on the device, F = pooled ? 1 : B, a row = HE (6,
 * row-major), P (6, row-major), maxC (2), n, valid.  A fit is INVALID (valid = 0, n kept, the rest zero) when n < 16, det(HE^T HE) is
 * not > 1e-12 or a maxC is not > 0: flagged, never a fault or a NaN.  workspace: plipmi_stain_workspace(B, H, W, step) bytes of the
 * caller's, 16-byte aligned; it holds nothing between calls.
 * plipmi_stain_apply: every pixel (not only the sampled ones) of image b by fit row b (n_fits == B) or row 0 (n_fits == 1):
 * C = P . lut[rgb], C2[j] = C[j] * (target maxC[j] / maxC[j]), out[c] = min(255, Io exp(-(HE_t[c][0] C2[0] + HE_t[c][1] C2[1])))
 * truncated to a byte; target_dev: double [8] on the device = the target's HE (6, row-major) and maxC (2).  An image whose fit is
 * invalid is copied unchanged.  dst: uint8 [B, H, W, 3] contiguous; dwords are stored where W % 4 == 0 and dst is 4-byte aligned, and
 * loaded where src, pitch_bytes and image_stride_bytes are multiples of 4 as well; bytes otherwise.
 * Both only enqueue: no synchronisation, no allocation; B == 0 launches nothing.  PLIPMI_ERR_INVALID with a message, before any
 * launch: a null pointer, H or W < 1, step < 1, pitch_bytes < 3 W, an image of 2 GiB or more, more than 2^31 - 8193 sampled pixels
 * in a call, n_fits neither 1 nor B, alpha outside (0, 50), Io or beta not positive, a double buffer that is not 8-byte aligned. */
size_t plipmi_stain_workspace(int B, int H, int W, int step);   /* 0 for sizes the fit refuses */
int plipmi_stain_fit(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes, int step,
                     int pooled, double Io, double alpha, double beta, const double* lut_dev, void* workspace, double* fits_out,
                     void* stream);
int plipmi_stain_apply(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes,
                       const double* fits, int n_fits, const double* target_dev, double Io, const double* lut_dev, uint8_t* dst,
                       void* stream);

/* ---- bags of embeddings: slide-level top-K pooling and bag means ----------------
 * (Additive, like the entries above it: the version number and every existing entry are unchanged; a caller probes for the symbols.)
 * A BAG is a contiguous row range of X fp32 [N, D] (device, 16-byte aligned, D % 4 == 0, 4 <= D <= 1024): bag b is rows
 * [offsets[b], offsets[b + 1]), offsets int32 [S + 1] on the device, non-decreasing, offsets[0] = 0, offsets[S] = N; empty bags are
 * allowed.  The C entries cannot see the contents of offsets: the kernels clamp what they read to [0, N] and to non-decreasing values, so
 * no access leaves X or the outputs whatever the array holds (rows that then belong to no bag are ignored); the Python layer validates
 * them.  The definition is the project's own (tests/bags_common.py is its numpy statement; csrc/bags.hip):
 *   scores    s[c, i] = scale * (x_i . t_c) for T fp32 [C, D] (device, 16-byte aligned), 1 <= C <= PLIPMI_BAG_MAX_CLASSES; rows are used
 *             as given (unit rows for cosine).  Exact-fp32 MFMA products, the same tile and the same per-row order of the columns for
 *             every row: a row's score bits do not depend on N, on its bag or on the other bags of the call.  Class-major [C, N].
 *   order     (v, i) ranks before (w, j) iff v > w, or v == w and i < j (ties go to the lower row); -0.0 and +0.0 are equal; a NaN
 *             score counts as -inf.
 *   pooling   ks: 1 .. PLIPMI_BAG_MAX_KS strictly ascending values in 1 .. PLIPMI_BAG_MAX_K on the HOST, kmax = the last.  For bag b of
 *             n_b rows, class c and k, m = min(k, n_b):  pooled[b, j, c] = (float)(the sum of the m first-ranked scores / (double)m),
 *             the sum in float64 rank by rank (first-ranked first); NaN for an empty bag.
 *             The selection is exact.
 *   pred      pred[b, j] = the first arg-max over c of pooled[b, j, :] (a NaN never wins over a number); -1 for an empty bag.
 *   top_idx   top_idx[b, c, r] = the row of X (int32) of rank r < min(kmax, n_b), -1 beyond; an index written lies inside its bag.
 *   mean      mean[b, :] = (float)(the float64 sum of the bag's rows / n_b), the sum in a fixed association of ascending rows; with
 *             normalize, that fp32 row divided by its norm (float64); zeros for an empty bag or a zero norm.
 * No floating-point atomics, every sum in a fixed order: the same inputs give the same bits on every run.
 * plipmi_bag_topk_pool: the score pass, then the pooling of those scores; scores_out (fp32 [C, N], may be NULL) keeps them.
 * plipmi_bag_pool_scores: the same pooling of any class-major per-tile scores scoresT [C, ld], ld >= N -- the transposed output of
 * plipmi_logits, a probe's decision values.  pooled fp32 [S, nks, C]; pred int32 [S, nks] and top_idx int32 [S, C, kmax] may be NULL.
 * plipmi_bag_mean: mean fp32 [S, D].
 * All three only enqueue: no synchronisation, no allocation, no host work per bag, and a grid that depends on N, S, C alone (bag sizes
 * are read on the device), so the calls can be captured in a graph.  workspace: plipmi_bag_workspace bytes of the caller's (for
 * plipmi_bag_mean those of C = 1, kmax = 1 suffice), 16-byte aligned; it holds nothing between calls.
 * PLIPMI_ERR_INVALID with a message that names the limit, before any launch: a null required pointer, S < 1, C outside 1 .. 64, nks
 * outside 1 .. 8, a k outside 1 .. 1024, ks not strictly ascending, ld < N, a misaligned X, T or workspace, N < 1, D % 4, D outside
 * 4 .. 1024. */
#define PLIPMI_BAG_MAX_K 1024
#define PLIPMI_BAG_MAX_KS 8
#define PLIPMI_BAG_MAX_CLASSES 64
size_t plipmi_bag_workspace(int N, int S, int C, int kmax);   /* 0 for sizes the entries refuse */
int plipmi_bag_topk_pool(plipmi_handle h, const float* X, int N, int D, const int32_t* offsets, int S, const float* T, int C, float scale,
                         const int32_t* ks_host, int nks, void* workspace, float* pooled /*[S,nks,C]*/, int32_t* pred /*[S,nks] or NULL*/,
                         int32_t* top_idx /*[S,C,kmax] or NULL*/, float* scores_out /*[C,N] or NULL*/, void* stream);
int plipmi_bag_pool_scores(plipmi_handle h, const float* scoresT, int64_t ld, int N, int C, const int32_t* offsets, int S,
                           const int32_t* ks_host, int nks, void* workspace, float* pooled, int32_t* pred, int32_t* top_idx, void* stream);
int plipmi_bag_mean(plipmi_handle h, const float* X, int N, int D, const int32_t* offsets, int S, int normalize, void* workspace,
                    float* mean /*[S,D]*/, void* stream);

/* ---- measurement ------------------------------------------------------------
 * (kernel-level test entries and A/B hooks live in plipmi_test.h: same library, not part of the product interface) */
/* Per-kernel timing with HIP events recorded on the launch stream.  While
 * enabled every kernel launch of the handle is bracketed by two events; the
 * totals are read back (this call synchronises) as rows of `plipmi_kernel_stat`. */
typedef struct plipmi_kernel_stat {
  char   name[96];     /* kernel symbol family, e.g. "gemm_nt<bf16,128x128,bias_qgelu>" */
  int64_t calls;
  double total_ms;     /* sum of event-measured durations */
  double flops;        /* algorithmic FLOPs of those calls (GEMM/attention), 0 for byte-bound kernels */
  double bytes;        /* algorithmic bytes moved by those calls */
} plipmi_kernel_stat;
int plipmi_profile_enable(plipmi_handle h, int on);   /* on=1 starts (and clears), on=0 stops */
int plipmi_profile_read(plipmi_handle h, plipmi_kernel_stat* rows, int max_rows, int* n_rows);

#ifdef __cplusplus
}
#endif
#endif /* PLIPMI_H */
