/* vlatouch.h — C ABI of libvlatouch_hip.so, the MI355X (gfx950) engine behind the VLA-Touch
 * action-refinement path.
 *
 * The reference (jxbi1010/VLA-Touch) has no FFI: its boundary for this path is the Python class
 * surface of VLA/residual_controller/ and VLA/models/ (SURVEY.md §8b).  Those classes are mirrored in
 * vla-touch_amd/{residual_controller,models}/ and bind to the entry points below through ctypes
 * (vla-touch_amd/vlatouch/_lib.py).  Each entry cites the reference interface it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (PyTorch allocations) unless
 * marked "host"; no entry allocates device memory, synchronises the device or touches the default
 * stream — all work is enqueued on `stream` (a hipStream_t).  Return value: 0 on success, negative
 * errno-style code otherwise (-22 bad argument, -95 unsupported, -5 launch failure);
 * vt_last_error() returns a host string for the last failure on the calling thread.
 * dtype codes: 0 = fp32, 1 = bf16 (raw 16-bit), 2 = fp32 storage with split-bf16 compute (GEMM weights only), 3 = IEEE fp16.
 * "cdt" = compute/storage dtype of weights,
 * "adt" = dtype of activations between kernels.
 */
#ifndef VLATOUCH_H
#define VLATOUCH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* vt_stream_t;   /* hipStream_t */
typedef struct vt_unet_s* vt_unet_t;
typedef struct vt_dino_s* vt_dino_t;
typedef struct vt_lstm_s* vt_lstm_t;
typedef struct vt_rdt_s* vt_rdt_t;
typedef struct vt_t5_s* vt_t5_t;

const char* vt_last_error(void);
int vt_version(void);
/* MFMA fragment-layout self test (A = I with asymmetric B, both dtypes); out_err[2] device floats. */
int vt_selftest_mfma(float* out_err, vt_stream_t stream);

/* Live timing of the LDS-DMA MFMA GEMM kernels: while enabled, every launch of the selected kernel class is bracketed by HIP
 * events on its launch stream.  on = 0 off, 1 every GEMM class, 2 only the 256-square ping-pong tiles (gemm_pp256d_kernel,
 * gemm_pt_kernel), 3 only the 128- / 160-column tiles (gemm_glds_kernel, gemm_ppk_kernel, gemm_pw_kernel, gemm_pws_kernel),
 * 4 only the cached cross-attention, 5 only the register-staged GEMMs, 6 only the fused U-Net convolution.  vt_prof_collect (after the caller synchronised the stream) returns the
 * summed duration, the algorithmic FLOPs / bytes of those launches and their count. */
int vt_prof_enable(int on);
int vt_prof_collect(double* total_ms, double* flops, double* bytes, long* launches);

/* ---------------------------------------------------------------- primitives (unit-test hooks) */
/* Generic GEMM / implicit conv1d: params = struct VtGemmParams (csrc/vt_gemm.h), host pointer.
 * Replaces torch nn.Linear / nn.Conv1d / nn.ConvTranspose1d calls of
 * bridge/networks/conditional_unet_1D.py:25,34,49,83, bridge_controller.py:42-48, HF Dinov2 linears. */
int vt_gemm(const void* params, vt_stream_t stream);
/* Which kernel vt_gemm runs for a parameter block (csrc/vt_gemm_route.hip: the one function that decides; host code only, nothing is launched, no
 * GPU is needed).  VT_ROUTE_ROWSPLIT = two launches: the full 256-row blocks on the 256-square tile (head: VT_ROUTE_PT or VT_ROUTE_PP) and the
 * remaining <= 64 rows as a launch of their own (tail: any route); vt_gemm_route_split reports both for a block that routes there (else -22). */
enum { VT_ROUTE_UNSUPPORTED = 0,   /* vt_gemm returns -95 */
       VT_ROUTE_BAD_ARG = 1,       /* vt_gemm returns -22 */
       VT_ROUTE_REG = 2,           /* register-staged gemm_kernel (csrc/vt_gemm.hip) */
       VT_ROUTE_F32R = 3,          /* exact-fp32 LDS-DMA ring, gemm_f32r_kernel */
       VT_ROUTE_GLDS = 4,          /* 128-column LDS-DMA tile, gemm_glds_kernel */
       VT_ROUTE_PP = 5,            /* 256-square ping-pong tile, gemm_pp256d_kernel */
       VT_ROUTE_PT = 6,            /* its persistent form, gemm_pt_kernel */
       VT_ROUTE_PPK = 7,           /* 160 x 128 split-K tile, gemm_ppk_kernel */
       VT_ROUTE_PW = 8,            /* weights-in-registers tile, gemm_pw_kernel */
       VT_ROUTE_PWS = 9,           /* small-M packed tile, gemm_pws_kernel */
       VT_ROUTE_ROWSPLIT = 10 };
int vt_gemm_route_of(const void* params);
int vt_gemm_route_split(const void* params, int* head_route, int* tail_route);
/* Frozen 16-bit weights W [N][K] (row stride ldw) -> a second copy in MFMA fragment order [N/32][K/16][64 lanes][8] (N % 32 == 0,
 * K % 16 == 0; same byte count): VtGemmParams.Wp of the weights-in-registers GEMM tile (csrc/vt_gemm_pw.hip).  Replaces nothing in
 * the reference (torch.nn.Linear keeps one layout, models/rdt/blocks.py:144-183); it is the load-time packing of this engine. */
int vt_pack_w32(const void* W, long ldw, void* out, int N, int K, vt_stream_t stream);
/* Kernel selection knobs of the dispatcher (tests, tools/): knob 1 = ring depth of the weights-in-registers tile (0 default, 4, 8);
 * knob 2 = that tile on (1) / off (0); knob 4 = k-split factor of the small-M tile (csrc/vt_gemm_pws.hip; 0 = none, -1 = choose);
 * knob 6 = fixed-maximum softmax of the cached cross-attention on (1) / off (0: always the online form);
 * knob 7 = fused U-Net sampler path (vt_unet_fused_pack) on (1) / off (0: the launch-per-op driver);
 * knob 8 = persistent 256-square GEMM tile with the in-loop epilogue (csrc/vt_gemm_pt.hip) on (1) / off (0: gemm_pp256d_kernel);
 * knob 9 = grouped-query ViT self-attention (csrc/vt_attn.hip, attn16g_kernel: a block walks the keys once for G x 16 query rows per wave):
 *          0 off (attn16u_kernel), 1 = 64-wide heads with at most 384 query rows (DINOv2 @224; default), 3 / 6 = every 16-bit unmasked call, G pinned.
 * Any other knob (or value) returns VT_ERR_ARG. */
int vt_tune(int knob, int value);

/* Flash attention, head_dim 64 (or 96: params.hd): params = struct VtAttnParams (csrc/vt_kernels.h), host pointer.
 * Replaces F.scaled_dot_product_attention (models/rdt/blocks.py:116-123) and HF Dinov2SelfAttention.  A query row whose keys are all masked
 * (kmask) is written as zeros, where torch's SDPA returns NaN: the row vt_attention_bwd gives zero gradients. */
int vt_attention(const void* params, vt_stream_t stream);
/* Cross-attention against a cached condition, head_dim 64, bf16 or fp16: params = struct VtAttnKvtParams (csrc/vt_kernels.h), host pointer.
 * K / V come as the per-head tile stream documented in csrc/vt_attn_kvt.hip; params.parts > 1 splits every sample's keys over that many
 * blocks and needs params.part_ws of vt_attention_kvt_part_bytes(B, H, Nq, parts) bytes.  Replaces the SDPA call of CrossAttention.forward
 * (models/rdt/blocks.py:102-123) against the image / language condition. */
int vt_attention_kvt(const void* params, vt_stream_t stream);
size_t vt_attention_kvt_part_bytes(int B, int H, int Nq, int parts);
/* Row-major K and V [M][ld] (head h at columns h*64..) -> that tile stream KV, T tiles per head (T * 64 >= M, rows >= M zero). */
int vt_retile_kv(const void* K, const void* V, long ld, void* KV, int M, int T, int H, vt_stream_t stream);
/* GroupNorm(+Mish, FiLM, residual) over fp32 split-K slabs: params = struct VtGnParams. */
int vt_groupnorm(const void* params, vt_stream_t stream);
/* Row norm: mode 0 LayerNorm, 1 RMSNorm(mean-square), 2 RMSNorm(timm<=1.0.8 unbiased-variance form). */
int vt_rownorm(const void* x, int xdt, long ldx, void* y, int ydt, long ldy, const float* w, const float* b,
               int rows, int D, float eps, int mode, vt_stream_t stream);
/* controller_dataset.py:303-346 / :349-384 (padding factor 1.4): out = (de)normalise(in) per last-dim stats. */
int vt_action_normalize(const float* in, float* out, const float* mins, const float* maxs, long n, int dim,
                        float padding_factor, int denormalize, vt_stream_t stream);
/* N(0, 1) draws on the device (counter-based Philox4x32-10 + Box-Muller) for callers that do not inject noise: replaces torch.randn
 * (rdt_runner.py:136) / torch.randn_like (bridge_model.py:372).  state = 2 x uint64 in DEVICE memory {key, next counter}, advanced behind the
 * draw by a one-thread kernel (a captured graph draws fresh noise at every replay); round_bf16 != 0 rounds the values to the bf16 grid. */
int vt_randn(float* out, long n, void* state, int round_bf16, vt_stream_t stream);
/* out [B][T][Dd] fp32 = in[:, :T, :Dd] of in [B][Tin][Din] (idt fp32 / bf16): the slice + cast between the RDT chunk and the controller's
 * `vla_actions` (frank_inference_eef.py:495-517 does it with tensor indexing). */
int vt_slice_cast(const void* in, int idt, float* out, int B, int Tin, int Din, int T, int Dd, vt_stream_t stream);
/* out [rows][cols] (odt) = in (idt), element-wise dtype conversion with row strides (fp32 / bf16 / fp16): `.to(dtype)` between pipeline
 * stages, e.g. SigLIP image tokens -> RDTRunner.predict_action's img_tokens (franka_model_eef.py:286-288). */
int vt_cast(const void* in, int idt, long ldi, void* out, int odt, long ldo, int rows, int cols, vt_stream_t stream);

/* ---------------------------------------------------------------- interpolant U-Nets + SDE sampler
 * Replaces InterpolantsConditionalUnet1D / DiffusionConditionalUnet1D.forward
 * (bridge/networks/conditional_unet_1D_si.py:4-50, conditional_unet_1D.py:194-247) and
 * StochasticInterpolants.sample / sde_vs (bridge/bridge_model.py:259-279, 334-387).
 * A handle evaluates `nets` (1 or 2) structurally identical U-Nets on the same input in grouped launches
 * (the sampler uses 2 = {v_net, s_net}); weights are packed [nets][...] per layer by the caller in the
 * order documented in csrc/vt_unet.hip (`vt_unet_weight_order`). */
typedef struct {
  int nets;            /* 1 or 2 */
  int input_dim;       /* 10 */
  int input_pad;       /* input_dim rounded up to 16 */
  int cond_dim;        /* global_cond_dim (256) */
  int dsed;            /* diffusion_step_embed_dim (256) */
  int n_groups;        /* 8 */
  int ksize;           /* 5 */
  int n_levels;        /* 3 */
  int dims[4];         /* down_dims */
  int cdt;             /* weight dtype */
  int adt;             /* activation dtype */
} vt_unet_desc;
int vt_unet_create(const vt_unet_desc* desc, const void* const* weights, int n_weights, vt_unet_t* out);
void vt_unet_destroy(vt_unet_t h);
int vt_unet_num_weights(const vt_unet_desc* desc);
size_t vt_unet_workspace_bytes(vt_unet_t h, int B, int T);
/* out[nets][B][T][input_dim] fp32 = net_i(x, t, cond); t = per-sample timesteps t_dev[B] (device) or, if
 * t_dev == NULL, the scalar t_host for every sample. */
int vt_unet_forward(vt_unet_t h, const float* x, const float* t_dev, float t_host, const float* cond,
                    float* out, int B, int T, void* workspace, vt_stream_t stream);
/* Forward velocity-score SDE (sde_vs, direction='forward', score_weight 1): x[B][T][dim] fp32 is updated in
 * place through n_steps Euler–Maruyama steps; noise = N(0,1) draws [n_steps][B][T][dim] (the reference's
 * torch.randn_like sequence) or NULL for the deterministic drift; traj (optional) receives the n_steps+1
 * states.  Schedules are the reference's string-keyed ones (bridge_model.py:59-101):
 *   gamma_type   0 '2^0.5*t(t-1)'   1 '(2t(t-1))^0.5'   2 '(1-t)^2(2t)^0.5'
 *   epsilon_type 0 '1-t'   1 't(t-1)'   2 '1-sqrt(t)'   3 '1-t^2'   4 '0'
 *   sde_type     0 'vs' (nets = {v_net, s_net}, sde_vs :334-387)   1 'bs' (nets = {b_net, s_net}, sde_bs :281-332) */
int vt_si_sample(vt_unet_t h, float* x, const float* cond, const float* noise, int n_steps, float beta_max,
                 int gamma_type, int epsilon_type, int sde_type, float* traj, int B, int T, void* workspace,
                 vt_stream_t stream);
/* The same with the two remaining arguments of sde_vs / sde_bs (bridge_model.py:281, 334): backward != 0 = direction='backward' (nets and
 * schedules evaluated at 1 - t, x <- x - (b - w eps s) dt, :356-361, :379-382; the epsilon inside b stays at t as :369 writes it),
 * score_weight = w (:376).  vt_si_sample == vt_si_sample_ex(..., 0, 1.0f, ...). */
int vt_si_sample_ex(vt_unet_t h, float* x, const float* cond, const float* noise, int n_steps, float beta_max,
                    int gamma_type, int epsilon_type, int sde_type, int backward, float score_weight, float* traj,
                    int B, int T, void* workspace, vt_stream_t stream);
/* Fused sampler path (csrc/vt_uconv.hip, vt_unet_fused.hip): in the split-bf16 mode (cdt = VT_F32X3, adt = VT_F32, dims % 64 == 0)
 * every Conv1d resolves GroupNorm + Mish + FiLM + residual of its input in its own prologue — 30 launches per SDE step instead of 67.
 * It needs a second copy of the convolution weights as pre-split bf16 hi / lo in MFMA fragment order: vt_unet_fused_bytes = size of
 * that buffer (0 = configuration not supported), vt_unet_fused_pack fills it on the device and switches vt_si_sample* (and
 * vt_unet_forward with a scalar time) of the handle to the fused path.  The buffer must outlive the handle. */
size_t vt_unet_fused_bytes(vt_unet_t h);
int vt_unet_fused_pack(vt_unet_t h, void* buf, vt_stream_t stream);
/* 1 when vt_si_sample* / vt_unet_forward of this handle take the fused path at (B, T, n_steps): packed weights present, T halves cleanly down the
 * levels (T <= 64: 16, 32, 48, 64, 24 ...; 48-tick chunks are what scripts/franka_inference_eef.py refines), every convolution of the plan finds a
 * tile and the final kernel's LDS fits the CU.  0 = the launch-per-op driver runs (same results).  vt_unet_workspace_bytes covers both. */
int vt_unet_fused_covers(vt_unet_t h, int B, int T, int n_steps);
/* Workspace bytes of the fused plan at (B, T, n_steps); 0 = the plan cannot run this shape or configuration.  Host-only (no launch, independent
 * of vt_unet_fused_pack): what vt_unet_fused_covers decides on, and part of vt_unet_workspace_bytes. */
size_t vt_unet_fused_plan_bytes(vt_unet_t h, int B, int T, int n_steps);
/* In-place per-head RMSNorm over 64-wide head slices (timm Attention q_norm/k_norm, models/rdt/blocks.py:150-156):
 * x[token*tok_stride + head*64 + 0..63], mode as vt_rownorm (1 or 2). */
int vt_headnorm(void* x, int dt, long tok_stride, int heads, long tokens, const float* w, float eps, int mode,
                vt_stream_t stream);

/* ---------------------------------------------------------------- DINOv2 CLS encoder
 * Replaces DINOv2Encoder.forward/_normalize_images (residual_controller/visual_encoder.py:56-106) and the
 * HF Dinov2Model forward it calls.  `ncams` image batches (each B images) are preprocessed with their OWN
 * max()/mean() decisions (one reference call per camera, bridge_controller.py:106-107) and then run through
 * the transformer as one batch of ncams*B. */
typedef struct {
  int hidden, layers, heads, patch, kpad;   /* kpad = 3*patch*patch rounded up to 16 (592) */
  int cdt, adt;
  float eps;
  /* ViT variants beyond DINOv2 (all 0 = DINOv2): SigLIP has no CLS token, tanh-GELU, 72-wide heads packed zero-padded to 96,
   * an FFN width that is not 4*hidden, and returns every token after the final LayerNorm */
  int no_cls;        /* 1: no CLS token (tokens = patches) */
  int act;           /* 0: erf GELU (VT_ACT_GELU_ERF); else a VT_ACT_* code; 5 (VT_ACT_SWIGLU) = dinov2-giant's gated FFN: fc1 = weights_in
                        [2*mlp_dim][hidden] -> silu(x1) * x2 -> fc2 = weights_out [hidden][mlp_dim] (HF Dinov2SwiGLUFFN) */
  int head_dim;      /* 0 / 64, or 96 (attention width heads*head_dim; weights packed accordingly) */
  int mlp_dim;       /* 0: 4*hidden; else the (64-padded) FFN width */
  int out_all;       /* 0: out = [ncams][B][hidden] CLS rows; 1: out = [ncams][B][tokens][hidden] */
  float attn_scale;  /* 0: head_dim^-0.5 */
  /* CLIP vision tower with deep visual prompts (Octopi's tactile encoder; all 0 = the variants above).  With act = 7 (VT_ACT_QUICK_GELU),
   * ones for the two LayerScale slots and a zero patch bias this is HF CLIPVisionTransformer; out_all = 0 gives pooler_output. */
  int pre_ln;        /* 1: LayerNorm of every embedded row (CLIP pre_layrnorm) before block 0; two weights (gain, bias) follow the final norm's */
  int n_prompt;      /* n_ctx learnable prompt rows appended after the patch tokens of every image (needs a CLS token) */
  int prompt_depth;  /* P: blocks 0 .. P-1 see the prompt rows, block P drops them; -1 = every block; 0 = no prompts (n_prompt is ignored).
                        Weights after the pre_ln pair when P != 0 and n_prompt > 0: VPT [n][hidden] fp32, VPT_shallow_i [n][hidden] fp32 for
                        1 <= i < P, then ONE fp32 array [layers] of the gates sigmoid(VPT_gamma_i) at index i (only 1 <= i < P, i != last are read) */
  int image_size;    /* != 0: vt_dino_forward / vt_dino_embed refuse any other `res` (CLIP's position table is never interpolated) */
} vt_dino_desc;
int vt_dino_create(const vt_dino_desc* desc, const void* const* weights, int n_weights, vt_dino_t* out);
void vt_dino_destroy(vt_dino_t h);
int vt_dino_num_weights(const vt_dino_desc* desc);
size_t vt_dino_workspace_bytes(vt_dino_t h, int B_total, int res);
/* Optional fragment-packed second copies of the fc1 weights (vt_pack_w32 layout; 16-bit modes, GELU FFN): the caller allocates vt_dino_packed_bytes(h) bytes
 * (0 = not applicable) and keeps them resident; vt_dino_set_packed enqueues the packing kernels.  With them the rows a 256-row tiling of the token matrix leaves
 * over, and the CLS-only last block, run fc1 on the small-M packed-weight tile.  Replaces nothing in the reference (a layout of its nn.Linear weights). */
size_t vt_dino_packed_bytes(vt_dino_t h);
int vt_dino_set_packed(vt_dino_t h, void* buf, vt_stream_t stream);
int vt_dino_set_range_flag(vt_dino_t h, unsigned* word);      /* see vt_rdt_set_range_flag */
/* imgs[ncams] device pointers; is_u8: uint8 pixels else fp32; nhwc: [B,H,W,3] else [B,3,H,W];
 * pre_scale: 1/255 when the caller passed a numpy array (visual_encoder.py:66) else 1;
 * norm_mode: 0 auto (reference behaviour), 1 force ImageNet-normalise, 2 never; in all three a camera batch whose largest value
 *   (times pre_scale) exceeds 1 is divided by 255 (visual_encoder.py:78).  3 raw: scale = pre_scale, no such rule and no normalisation: the
 *   pixel values reach the patch embedding as they are (the SigLIP tower, whose image processor has already rescaled and normalised them;
 *   the statistics kernels still run and report max and mean);
 * pos_patch: [grid*grid][hidden] fp32 position embeddings already interpolated for `res`;
 * out: [ncams][B][hidden] fp32 pooler_output; flags_out (optional) [ncams][4] = {scale, normalised, max, mean}. */
int vt_dino_forward(vt_dino_t h, const void* const* imgs, int ncams, int is_u8, int nhwc, float pre_scale,
                    int norm_mode, int B, int res, const float* pos_patch, float* out, float* flags_out,
                    void* workspace, vt_stream_t stream);
/* The front end of vt_dino_forward alone, through the same code: statistics, patchify, patch-embed GEMM + position embedding, CLS row.
 * Same image arguments and workspace (vt_dino_workspace_bytes); tokens: [ncams*B][tokens][hidden] fp32, the residual stream as the first
 * block receives it, written straight into the caller's buffer; flags_out as above.  For a CLIP handle `tokens` counts the prompt rows too:
 * 1 + grid^2 + n_prompt rows per image when prompt_depth != 0 (VPT after the patch rows), every row after pre_layrnorm. */
int vt_dino_embed(vt_dino_t h, const void* const* imgs, int ncams, int is_u8, int nhwc, float pre_scale,
                  int norm_mode, int B, int res, const float* pos_patch, float* tokens, float* flags_out,
                  void* workspace, vt_stream_t stream);

/* ---------------------------------------------------------------- deep visual prompts of the CLIP tower (csrc/vt_prompt_seam.hip)
 * The two launches vt_dino_forward issues between blocks when n_prompt > 0, as entries (tests call them alone).  Replaces the prompt steps
 * of PromptLearningCLIPEncoderLayer.forward (octopi_s/utils/encoder.py:59-91, 108-124), vision branch.
 * vt_prompt_seam: on the last n rows of each of the Bt images of the fp32 residual stream tok [Bt][rows][D], per element and in this order:
 *   gate  (gate != null):    v = g * v + (1 - g) * before, g = *gate (DEVICE fp32 scalar), each product and the sum rounded to fp32;
 *   save  (save != 0):       before = v;
 *   overwrite (shallow != null): v = shallow [n][D];
 * `before` is [Bt][n][D] fp32 and must be given when gate or save is.  Rows outside the tail are neither read nor written.
 * tok, before and shallow are read and written as 16-byte vectors: they must be 16-byte aligned (as must src and dst of vt_prompt_compact).
 * Refused (-22) before any launch: null tok, Bt / n / D < 1, n > rows, D % 4, gate or save without before, nothing to do, a misaligned pointer.
 * vt_prompt_compact: [Bt][rows][D] -> [Bt][rows - n][D], the last n rows of every image dropped.  dst == src works in place (one workgroup
 * walks the images front to back); otherwise the two buffers must not overlap.  Refused (-22): null pointer, Bt / D < 1, n < 1, n >= rows, D % 4, a misaligned pointer. */
int vt_prompt_seam(float* tok, int Bt, int rows, int n, int D, const float* gate, float* before, int save, const float* shallow,
                   vt_stream_t stream);
int vt_prompt_compact(const float* src, float* dst, int Bt, int rows, int n, int D, vt_stream_t stream);

/* ---------------------------------------------------------------- tactile video heads (csrc/vt_tactile_head.hip)
 * Replaces ViFiCLIP.forward's video feature (encoder.py:401-411: mean over the l frames, then / L2 norm, no eps) and the retrieval of
 * dataset.py:189-195 (nn.CosineSimilarity(dim=1, eps=1e-8) of a saved bank against it, then torch.topk), batched over b videos that all
 * use the same bank.  pooled [b][l][D] fp32; video [b][D] fp32.  With bank != null ([R][D] fp32; bank_norm [R] fp32 = its rows' L2 norms,
 * vt_tactile_bank_norms): sims [b][R] fp32 = bank_r . video / (max(|bank_r|, 1e-8) * max(|video|, 1e-8)), and with k > 0 topk_idx int32
 * [b][k] / topk_val fp32 [b][k], the k largest similarities of each video in descending order; TIES GO TO THE LOWER INDEX.  Every sum is
 * taken in fp32 in an order that depends on l, D and R only, so a video's results do not depend on b.  A video whose mean feature is zero
 * has NaN for its feature and similarities (the reference divides without an eps); its top-k then lists the lowest indices 0 .. k-1 with NaN
 * values, always valid indices.  bank and video are read as 16-byte vectors and must be 16-byte aligned.
 * Refused (-22) before any launch: null pooled / video, b / l / D < 1, D % 4, a bank without bank_norm or sims, R < 1, k < 0, k > R, k > 16,
 * k > 0 without topk_idx / topk_val, a misaligned bank or video. */
int vt_tactile_bank_norms(const float* bank, int R, int D, float* bank_norm, vt_stream_t stream);
int vt_tactile_head(const float* pooled, int b, int l, int D, const float* bank, const float* bank_norm, int R, int k,
                    float* video, float* sims, int* topk_idx, float* topk_val, vt_stream_t stream);

/* ---------------------------------------------------------------- T5 v1.1 text encoder (csrc/vt_t5.hip)
 * Replaces HF T5EncoderModel (feed_forward_proj "gated-gelu") of models/multimodal_encoder/t5_encoder.py::T5Embedder, used by
 * scripts/encode_lang*.py and franka_model_eef.py (encode_instruction): instruction tokens -> last_hidden_state = RDT's lang_tokens.
 * d_kv must be 64; cdt = adt = 0 (fp32) or 1 (bf16 weights and GEMM operands; fp32 residual stream and accumulation).  There is no fp16 mode.
 * Weights (vt_t5_num_weights of them): shared [vocab][d_model] cdt, relative_attention_bias of layer 0 [num_buckets][heads] fp32, per layer
 * {layer_norm [d_model] fp32, q|k|v [3 heads*64][d_model] cdt, o [d_model][heads*64] cdt, layer_norm [d_model] fp32, wi_0|wi_1 [2 d_ff][d_model] cdt,
 * wo [d_model][d_ff] cdt}, final_layer_norm [d_model] fp32. */
typedef struct {
  int vocab, d_model, heads, d_kv, d_ff, layers;
  int num_buckets, max_distance;     /* relative_attention_num_buckets / relative_attention_max_distance (used by the host's bucket table) */
  float eps;                         /* layer_norm_epsilon */
  int cdt, adt;
} vt_t5_desc;
int vt_t5_create(const vt_t5_desc* desc, const void* const* weights, int n_weights, vt_t5_t* out);
void vt_t5_destroy(vt_t5_t h);
int vt_t5_num_weights(const vt_t5_desc* desc);
size_t vt_t5_workspace_bytes(vt_t5_t h, int B, int L);
/* ids: HOST int32 [B][L] token ids; mask_or_null: HOST uint8 [B][L] attention_mask (1 = token, 0 = padding; null = all tokens) — both are
 * validated on the host (an id outside [0, vocab) or a row with no valid token is -22) and copied into the workspace on `stream`.
 * L <= 1024.  bucket_tab: device int8 [2047], the relative-position bucket of rel = -1023 .. 1023 at index rel + 1023 (HF
 * T5Attention._relative_position_bucket, bidirectional, computed on the host in fp32).  out: [B][L][d_model] of out_dt (0 fp32, 1 bf16). */
int vt_t5_forward(vt_t5_t h, const int32_t* ids, const uint8_t* mask_or_null, int B, int L, const int8_t* bucket_tab, void* out, int out_dt,
                  void* workspace, vt_stream_t stream);
/* The encoder's own two kernels as entries (tests call them alone; vt_t5_forward launches them through these and in no other way).
 * vt_t5_attention: out = softmax(q k^T + rel_bias[bucket(j - i)][h], masked keys at -inf) v per (batch, head), head width 64, NO 1/sqrt(d)
 * scale.  All pointers are DEVICE pointers.  qkv [B*L][3*H*64] (q | k | v, head h at column h*64 of its part), out [B*L][H*64], both of dt
 * (0 fp32, 1 bf16); bucket_tab int8 [2047] as vt_t5_forward takes it (entries are clamped to 0 .. num_buckets-1); rel_bias fp32
 * [num_buckets][H]; kmask_or_null uint8 [B][L], 1 = attend.  A sample without a valid key comes out as zeros (vt_t5_forward rejects one).
 * Refused before any launch: a null required pointer, B, H or L < 1, B or H > 65535, L > 1024, num_buckets outside 1 .. 127 (-22); any
 * other dt (-95).
 * vt_t5_geglu: h[r][c] = gelu_tanh(g[r][c]) * g[r][F + c] for c < F (HF gelu_new on the first half, the gate), out of place, rows of g ldg
 * elements apart and rows of h ldh apart, both DEVICE pointers aligned to 16 bytes, of dt (0 fp32, 1 bf16).  Refused before any launch: null
 * g or h, rows < 1, F < 1, F, ldg or ldh that is not a multiple of the 16-byte vector (4 fp32 or 8 bf16 elements), ldg < 2 F, ldh < F (-22);
 * any other dt (-95). */
int vt_t5_attention(const void* qkv, void* out, const int8_t* bucket_tab, const float* rel_bias, const uint8_t* kmask_or_null,
                    int B, int H, int L, int num_buckets, int dt, vt_stream_t stream);
int vt_t5_geglu(const void* g, long ldg, void* h, long ldh, long rows, int F, int dt, vt_stream_t stream);

/* ---------------------------------------------------------------- small MLP chain (state encoder / force encoder / heads)
 * y = L_n(...act(L_1(x))): replaces the nn.Sequential MLPs of bridge_controller.py:42-48 and
 * lstm_step_controller.py:44-60.  W_i [out_i][in_pad_i] cdt (in padded to 16), b_i fp32.  x is [B][ldx] of adt
 * with zero padding up to in_pad_1.  tmp: 2*B*max(out_i) adt elements. */
int vt_mlp(const void* x, long ldx, int B, int n_layers, const int* dims /* n_layers+1, padded ins */,
           const void* const* W, const float* const* b, int act, void* y, int ydt, long ldy,
           int cdt, int adt, void* tmp, vt_stream_t stream);
/* Gather [cls_cam1 | cls_cam2 | state | forces] rows into a zero-padded adt matrix (bridge_controller.py:129-132). */
int vt_concat_obs(const float* cls1, const float* cls2, int dv, const float* state, int sdim, const float* forces,
                  int fdim, void* out, int odt, long ldo, int B, vt_stream_t stream);

/* ---------------------------------------------------------------- LSTM residual head
 * Replaces TactileLSTMController.predict / predict_sequence / forward (lstm_step_controller.py:232-286, 288-319, 170-213):
 * force MLP -> L-layer LSTM cell with carried (h, c) -> [h_top | obs_cond] head -> vla_n + delta, as ONE persistent kernel for T
 * consecutive ticks (csrc/vt_lstm.hip).  hidden must be 256; weights pre-packed in MFMA fragment order by the host side
 * (order and layout: csrc/vt_lstm.hip above vt_lstm_create).  force_pad / in_pad are kept for ABI stability and ignored. */
typedef struct { int state_dim, hidden, layers, force_dim, force_pad, in_pad, cdt; } vt_lstm_desc;
int vt_lstm_create(const vt_lstm_desc* desc, const void* const* weights, int n_weights, vt_lstm_t* out);
void vt_lstm_destroy(vt_lstm_t h);
int vt_lstm_num_weights(const vt_lstm_desc* desc);
size_t vt_lstm_workspace_bytes(vt_lstm_t h, int B);
/* One tick: out_n[B][state_dim] = vla_n + delta (normalised); h, c: [layers][B][hidden] fp32, updated in place. */
int vt_lstm_step(vt_lstm_t hd, const float* obs_cond, const float* vla_n, const float* force, float* h, float* c,
                 float* out_n, int B, void* workspace, vt_stream_t stream);
/* T ticks in one launch: vla_n [B][T][state_dim], force [B][T][force_dim] -> out_n [B][T][state_dim]; (h, c) carried in LDS /
 * registers across the ticks, read at entry and written back at exit. */
int vt_lstm_sequence(vt_lstm_t hd, const float* obs_cond, const float* vla_n, const float* force, float* h, float* c,
                     float* out_n, int B, int T, vt_stream_t stream);

/* ---------------------------------------------------------------- RDT diffusion transformer + DPM-Solver++ sampler
 * Replaces RDT.forward (models/rdt/model.py:126-165; blocks models/rdt/blocks.py:72-202) and
 * RDTRunner.predict_action / conditional_sample / adapt_conditions (models/rdt_runner.py:108-165, 225-250).
 * head_dim must be 64; rms_mode as vt_rownorm (1 = mean-square, 2 = timm<=1.0.8 variance form).
 * Weight order: csrc/vt_rdt.hip header. */
typedef struct {
  int hidden, depth, heads, horizon, out_dim;
  int state_dim;        /* state_token_dim (128); the state adaptor takes 2*state_dim (state | mask) */
  int lang_dim, img_dim;
  int max_lang_len, img_len;
  int n_lang, n_img, n_state;   /* adaptor depths: 1 = 'linear', N = 'mlpNx_gelu' */
  int cdt, adt;                 /* both fp32 or both bf16 */
  int rms_mode;
} vt_rdt_desc;
int vt_rdt_create(const vt_rdt_desc* desc, const void* const* weights, int n_weights, vt_rdt_t* out);
void vt_rdt_destroy(vt_rdt_t h);
int vt_rdt_num_weights(const vt_rdt_desc* desc);
size_t vt_rdt_workspace_bytes(vt_rdt_t h, int B, int lang_len);
/* The part of that workspace a caller driving vt_gemm itself needs for the small-M packed-weight tile (VtGemmParams.sk_ws / sk_cnt): bytes of
 * fp32 slabs for Linears of at most M rows and N columns (0 above 512 rows: nothing splits there), and the number of int32 ticket counters
 * (zeroed once by the caller, self-resetting afterwards).  Host only. */
size_t vt_splitk_slab_bytes(int M, int N);
int vt_splitk_counters(void);
/* Optional fragment-packed second copies of the Linears of the denoise loop (vt_pack_w32 layout; bf16, hidden % 512 == 0): the caller
 * allocates vt_rdt_packed_bytes(h) bytes (0 = not applicable), vt_rdt_set_packed enqueues the packing kernels and keeps the pointers. */
/* bounds[depth] (host): per block an upper bound of |q . k| * scale of its cross-attention (8 max|q_norm.weight| max|k_norm.weight| for the
 * mean-square RMSNorm of blocks.py:86-87; 0 = none) -> the cached cross-attention uses a fixed-maximum softmax where the bound is <= 40. */
int vt_rdt_set_score_bounds(vt_rdt_t h, const float* bounds, int n);
/* 16-bit mode only: 1 (default) = DPM-Solver++ state, x0 predictions and the final projection in fp32 between network evaluations; 0 = the
 * reference's bf16 rounding points (models/rdt_runner.py:137-139,160: `noisy_action.to(dtype)` after every scheduler step). */
int vt_rdt_set_state_precision(vt_rdt_t h, int fp32_state);
/* 16-bit modes: the reference's dtype when it differs from the engine's compute type (desc.cdt = desc.adt = VT_F16 evaluating a bf16 model with IEEE
 * fp16 activations — same width and MFMA rate, 3 more mantissa bits, the bf16 weights convert exactly): the start noise (models/rdt_runner.py:137-139)
 * and, with vt_rdt_set_state_precision(h, 0), the solver state are rounded to THIS grid.  VT_BF16 (default for bf16 engines) or VT_F16. */
int vt_rdt_set_io_dtype(vt_rdt_t h, int io_dtype);
size_t vt_rdt_packed_bytes(vt_rdt_t h);
int vt_rdt_set_packed(vt_rdt_t h, void* buf, vt_stream_t stream);
/* Range guard (round 6).  The reference executes RDT in bf16 (models/rdt_runner.py:47-60,160; models/rdt/model.py:124: 8 exponent bits); an engine created
 * with desc.cdt = desc.adt = VT_F16 has 5.  `word` = ONE zero-initialised uint32 in device memory, owned by the caller, resident as long as the handle is used
 * (NULL = detach).  The kernels of vt_rdt_sample / vt_rdt_forward OR bits into it — no extra launch, never cleared by the library, so it is sticky across calls
 * and hipGraph replays; the caller reads it when it likes (after a stream synchronise) and re-zeroes it:
 *   VT_RANGE_XN_SAT     the un-normalised 16-bit operand x * gain a residual Linear hands to the next Linear (csrc/vt_gemm_pw.hip) left the fp16 range and was clamped
 *   VT_RANGE_NONFINITE  an x0 prediction / solver state (vt_rdt_sample) or an output element (vt_rdt_forward) is inf or NaN: every other 16-bit store of the path
 *                       converts with v_cvt_f16_f32 (overflow -> inf), and inf / NaN propagate through every consumer (GEMMs, norms, softmax) into the fp32
 *                       residual stream, so an overflow anywhere upstream — inputs and converted weights included — ends here
 *   VT_RANGE_ATTN_EMPTY a cross-attention row whose probabilities summed to 0 or inf (all keys masked, or a degenerate score row); the row is written as zeros
 *                       (torch's SDPA returns NaN for a fully masked row, models/rdt/blocks.py:116-123)
 * vt_dino_set_range_flag: the same word for a DINOv2 / SigLIP handle — VT_RANGE_GATE_SAT: the gated SwiGLU product of dinov2-giant left the fp16 range and was clamped. */
#ifndef VT_RANGE_XN_SAT
#define VT_RANGE_XN_SAT 1u
#define VT_RANGE_NONFINITE 2u
#define VT_RANGE_GATE_SAT 4u
#define VT_RANGE_ATTN_EMPTY 8u
#endif
int vt_rdt_set_range_flag(vt_rdt_t h, unsigned* word);
/* RDT.forward: x_tokens [B][horizon+1][hidden] adt (adapted state + action tokens), freq [B] fp32, t = t_dev[B] or the
 * scalar t_host when t_is_scalar, lang_c [B][L][hidden] / img_c [B][img_len][hidden] adt (adapted, before position
 * embeddings), lang_mask [B][L] bytes (1 = valid) or NULL -> out [B][horizon][out_dim] adt. */
int vt_rdt_forward(vt_rdt_t h, const void* x_tokens, const float* freq, const float* t_dev, float t_host, int t_is_scalar,
                   const void* lang_c, const void* img_c, const uint8_t* lang_mask, void* out, int B, int L,
                   void* workspace, vt_stream_t stream);
/* RDTRunner.predict_action: lang_tokens [B][L][lang_dim], img_tokens [B][img_len][img_dim], state_tokens [B][1][state_dim],
 * action_mask [B][1][state_dim] (all adt), ctrl_freqs [B] fp32, x_init [B][horizon][state_dim] fp32 (the N(0,1) start the
 * reference draws with torch.randn), host arrays timesteps[n_steps] and coef[n_steps][5] = {a, b0, b1, alpha_s, sigma_s} of
 * the multistep update x <- a x + b0 x0_k + b1 x0_{k-1}; sample_pred: 1 = 'sample' prediction, 0 = 'epsilon'.
 * adapted != 0 = conditional_sample (rdt_runner.py:122): lang/img/state tokens are already adapted to [.., hidden].
 * out [B][horizon][state_dim] fp32 (values on the adt grid, masked). */
int vt_rdt_sample(vt_rdt_t h, const void* lang_tokens, const uint8_t* lang_mask, const void* img_tokens,
                  const void* state_tokens, const void* action_mask, const float* ctrl_freqs, const float* x_init,
                  int n_steps, const float* timesteps, const float* coef, int sample_pred, int adapted, float* out,
                  int B, int L, void* workspace, vt_stream_t stream);

/* ---------------------------------------------------------------- GelSight marker tracker -> m_t
 * Replaces EnhancedMarkerTracker.init_standard / detect_markers / match_and_compute_displacement / estimate_force
 * (residual_controller/tactile/marker/marker_tracker.py:81-114, 154-183, 308-341, 343-373) for a BATCH of frames.
 * frames [N][H][W][channels] bytes (channels 3 = BGR as cv2 delivers it, 1 = gray).  Per frame: 5x5 blur -> adaptive
 * Gaussian threshold (11, C = 2, inverted) -> 3x3 open -> outer contours of the 8-connected components -> polygon area in
 * (min_area, max_area) -> truncated polygon centroid, in cv2.findContours order (last found first).
 * markers [N][max_markers][2] int32 (x, y), counts [N] (may exceed max_markers or max_cand: overflow, the caller checks),
 * binary_out [N][H][W] bytes (0/1; the reference's `processed_frame` / 255) or NULL.
 * mode 0: gelsight_version 'standard' (init_standard).  mode 1: `frames` is already a processed binary image [N][H][W] (non-zero =
 * marker), only the contour stage runs (detect_markers :154).  mode 2: 'HSR' (init_HSR :116-152: invert, equalizeHist, 5x5 blur,
 * threshold > 50, 3x3 open).  mode | 0x100: BGR2GRAY with the 14-bit coefficient table of OpenCV <= 3.4.1 ((1868 B + 9617 G + 4899 R +
 * 8192) >> 14) instead of the 15-bit set of OpenCV >= 3.4.2 / 4.x ((3735 B + 19235 G + 9798 R + 16384) >> 15, the default: what the
 * reference's unpinned `opencv-python` resolves to). */
size_t vt_marker_workspace_bytes(int N, int H, int W, int max_cand);
int vt_marker_detect(const uint8_t* frames, int channels, int mode, int N, int H, int W, double min_area, double max_area,
                     int max_cand, int* markers, int* counts, int max_markers, uint8_t* binary_out, void* workspace,
                     vt_stream_t stream);
/* baseline [n_base][2] int32 -> disp [N][max_markers][2] int32 (marker - nearest baseline marker, ties to the lower index),
 * force [N][3] fp64 = |mean displacement|, unit direction x, y (zeros when no marker). */
int vt_marker_displacement(const int* markers, const int* counts, int N, int max_markers, const int* baseline, int n_base,
                           int* disp, double* force, vt_stream_t stream);

/* ---------------------------------------------------------------- controller training step primitives
 * Replace torch autograd / optim.AdamW / torch_ema around the interpolant losses (bridge/bridge_model.py:183-246 velocity_loss,
 * score_loss, b_loss, get_loss; bridge_train.py:49-58, 312-334).  fp32, channel-last [B][T][C]; the matrix products of the backward pass
 * are vt_gemm calls on the buffers these produce (vlatouch/train.py composes them; csrc/vt_train.hip). */
/* out[(tap*Cin + ci)][b*Tout + t] = x[b][t*stride + off0 + tap][ci] (0 outside): transposed im2col, the operand of a weight gradient */
int vt_im2col_t(const float* x, float* out, int B, int Tin, int Tout, int Cin, int taps, int stride, int off0, vt_stream_t stream);
int vt_transpose(const float* in, float* out, int M, int N, vt_stream_t stream);                 /* [M][N] -> [N][M] */
int vt_zero_stuff(const float* x, float* out, int B, int T, int C, vt_stream_t stream);           /* out[b][2u] = x[b][u], odd rows 0 */
int vt_wflip(const float* W, float* WT, int Cout, int taps, int Cin, vt_stream_t stream);         /* [Cout][taps][Cin] -> [Cin][taps reversed][Cout] */
int vt_colsum(const float* x, long ld, float* out, int M, int N, int accumulate, vt_stream_t stream);
int vt_add_(float* a, const float* b, long n, vt_stream_t stream);
int vt_copy_cols(const float* src, long lds, int off, float* dst, long ldd, int doff, int rows, int cols, int accumulate, vt_stream_t stream);
int vt_mish(const float* x, const float* dy, float* out, long n, vt_stream_t stream);             /* dy NULL: mish(x); else dy * mish'(x) */
/* backward of out = film_scale * mish(GroupNorm(c)) + film_bias: c, dout, dc [B*T][C]; film, dfilm [B][2C] (scale | bias) or NULL;
 * dgamma_part, dbeta_part [B][C] per-sample partials (sum over B with vt_colsum).  C / ngroups <= 256; a group (C / ngroups) * T of more than
 * 8188 elements (2 floats each + 32 bytes of static LDS past 64 KiB) returns VT_ERR_UNSUPPORTED. */
int vt_gn_mish_bwd(const float* c, const float* gamma, const float* beta, const float* film, const float* dout, float* dc,
                   float* dgamma_part, float* dbeta_part, float* dfilm, int B, int T, int C, int ngroups, float eps, vt_stream_t stream);
int vt_gelu(const float* x, const float* dy, float* out, long n, vt_stream_t stream);             /* erf GELU / its backward */
/* q_sample + the three loss targets of the LINEAR interpolant (bridge_model.py:103-107, 183-217, 248-258): xt, target_v = x1 - x0,
 * target_s = -z, target_b = (x1 - x0) + gamma'(t) z, t_clipped[B]; z already scaled by beta_max; gamma_type as vt_si_sample. */
int vt_si_qsample(const float* x0, const float* x1, const float* z, const float* t, float* xt, float* target_v, float* target_s,
                  float* target_b, float* t_clipped, int B, long per_sample, int gamma_type, float t_min, vt_stream_t stream);
/* the same for every `interpolant_type` of the reference (bridge_model.py:103-181: xt = w0(t) x0 + w1(t) x1 + gamma z, target_v = d(w0 x0 + w1 x1) / dt,
 * target_b = target_v + gamma'(t) z): 0 linear, 1 power3, 2 power4, 3 reverse_power3, 4 reverse_power4, 5 gaussian_encode_decode, 6 reverse_linear */
int vt_si_qsample_ex(const float* x0, const float* x1, const float* z, const float* t, float* xt, float* target_v, float* target_s,
                     float* target_b, float* t_clipped, int B, long per_sample, int gamma_type, float t_min, int interpolant_type, vt_stream_t stream);
/* loss[0] = mean_b(0.5 |out_b|^2 - <target_b, out_b>), dout = (out - target) / B   (the three interpolant losses share this form) */
int vt_si_loss(const float* out, const float* target, float* dout, float* loss, int B, long per_sample, vt_stream_t stream);
int vt_slab_sum(const float* slabs, int S, long n, const float* bias, int N, float* out, vt_stream_t stream);  /* split-K partials [S][n] -> out[n] (+ bias[i % N]) */
int vt_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
             int step, vt_stream_t stream);
int vt_ema_update(float* shadow, const float* p, long n, float decay, vt_stream_t stream);
/* the same two updates with the step-dependent scalars in DEVICE memory, hyper = [lr, 1 - beta1^t, sqrt(1 - beta2^t), 1 - ema_decay_t]:
 * a captured graph of the training step stays valid while t advances (the host rewrites 16 bytes before each replay) */
int vt_train_hyper(float lr, float beta1, float beta2, int step, float ema_decay, float* out4_host);   /* host-side: fills hyper for step t */
int vt_adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                 float weight_decay, vt_stream_t stream);
/* AdamW (+ EMA) over a device table of tensors in ONE launch.  table = ntensors records of 7 x 8 bytes:
 * {float* p, const float* g, float* m, float* v, float* shadow_or_null, int64 n, int64 first_chunk}, first_chunk = running sum of
 * ceil(n / 4096) over the preceding records; total_chunks = that sum over all records.  hyper as vt_adamw_dev. */
int vt_adamw_ema_multi(const void* table, int ntensors, long total_chunks, const float* hyper, float beta1, float beta2, float eps,
                       float weight_decay, vt_stream_t stream);
int vt_ema_update_dev(float* shadow, const float* p, long n, const float* hyper, vt_stream_t stream);
int vt_posemb(const float* t, float* out, int B, int dim, vt_stream_t stream);                    /* SinusoidalPosEmb: [sin | cos] */

/* ---- LSTM residual head training (lstm_step_controller.py:176-211 forward, :321-337 get_loss; lstm_train.py:26-33, 129-133).
 * Batch-major sequences [B][T][C]; `t` is the tick a call works on.  Gate order i, f, g, o (torch.nn.LSTM).
 * vt_lstm_cell_fwd: a = gx[b][t] (+ gh[b], required for t > 0) -> act[b][t][4H] (activated gates), cseq[b][t], hseq[b][t],
 *                   hprev[b][t+1] (= h_t; hprev[b][0] = 0), hcur[b] (contiguous copy of h_t).
 * vt_lstm_cell_bwd: dh = dhseq[b][t] (+ dh_rec[b], required for t < T-1); writes pre-activation gradients to dgates[b][t][4H] and
 *                   dgcur[b][4H]; dc_next[b] carries dL/dc between ticks (ignored on input at t = T-1).
 * vt_ln_bwd:        LayerNorm backward: dx, and dyxh = dy * x_hat whose column sums are d gamma (d beta = column sums of dy).
 * vt_bcast_mid / vt_sum_mid: dst[b][t][doff + c] = src[b][c] and its gradient out[b][c] = sum_t src[b][t][off + c].
 * vt_mse_residual:  pred = base + delta (base may be null), loss = mean((pred - target)^2), ddelta = 2 (pred - target) / n. */
int vt_lstm_cell_fwd(const float* gx, const float* gh, float* act, float* cseq, float* hseq, float* hprev, float* hcur, int B, int T, int H,
                     int t, vt_stream_t stream);
int vt_lstm_cell_bwd(const float* dhseq, const float* dh_rec, const float* act, const float* cseq, float* dc_next, float* dgates, float* dgcur,
                     int B, int T, int H, int t, vt_stream_t stream);
int vt_ln_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dyxh, int rows, int C, float eps, vt_stream_t stream);
int vt_bcast_mid(const float* src, float* dst, long ldd, int doff, int B, int T, int C, vt_stream_t stream);
int vt_sum_mid(const float* src, long lds, int off, float* out, int B, int T, int C, vt_stream_t stream);
int vt_mul_(float* a, const float* b, long n, vt_stream_t stream);
int vt_mse_residual(const float* base, const float* delta, const float* target, float* pred, float* ddelta, float* loss, long n, vt_stream_t stream);

/* ---- RDT fine-tuning step (csrc/vt_train_rdt.hip; vlatouch/rdt_train.py): the backward arithmetic of RDTRunner.compute_loss
 * (models/rdt_runner.py:168-222) through RDT.forward (models/rdt/model.py:126-165, blocks.py:72-202) and the clip of train/train.py:440-442.
 * Linears stay vt_gemm calls (data / weight gradients on transposed operands).
 * vt_attention_bwd: dQ, dK, dV of softmax(q k^T scale [+ key mask]) v (timm Attention / blocks.py:102-138 under autograd), head_dim 64,
 *   fp32 or bf16 operands with fp32 accumulation.  Q, dO, dQ are [B, Nq, H, 64] and K, V, dK, dV [B, Nk, H, 64] views given by element
 *   strides (batch, row, head; unit inner stride); kmask [B][km_bs] bytes (0 = key masked) or null.  The probabilities are recomputed; `ws`
 *   (B * H * Nq * 3 floats, device) receives the row statistics (max, 1 / sum, sum_j P dP).  No atomics: two calls give the same bits.  A query
 *   row with every key masked gets zero gradients, as a masked key does.
 * vt_rmsnorm_bwd: backward of vt_rownorm modes 1 / 2 (no bias), x, dy, dx, dyxr [rows][D] fp32; the column sums of dyxr (vt_colsum) are d w.
 * vt_headnorm_bwd: backward of vt_headnorm: x = the PRE-norm values, dy is overwritten by dx, both at [token * stride + head * 64 + 0..63];
 *   part [ceil(tokens * heads / 64)][64] partial sums of d w (vt_colsum finishes).
 * vt_act_bwd: act 2 = GELU(approximate="tanh") (timm Mlp, the adaptors), 3 = SiLU (TimestepEmbedder); dy null: act(x), else dy * act'(x).
 * vt_ddpm_qsample: DDPMScheduler.add_noise + the token layout of rdt_runner.py:197-204: out [B][horizon + 1][2A] = row 0: state ‖ mask,
 *   row 1 + r: sqrt(ab_t) action_r + sqrt(1 - ab_t) noise_r ‖ mask; alphas_cumprod [num_train_timesteps] fp32, timesteps [B] int64 (device).
 * vt_timestep_embed: blocks.py:41-61, out [B][dim] = cos(t f) | sin(t f) over the host's table f [dim / 2] = exp(-ln(10000) j / (dim / 2)).   vt_add_rowvec_: a[r][c] += v[c] (position embeddings).
 * vt_transpose_pad: [M][N] -> [N][Mp >= M], the padding columns zero (vt_gemm wants its reduction length as a multiple of 4).
 * vt_grad_clip_multi: torch.nn.utils.clip_grad_norm_ over the table of vt_adamw_ema_multi: chunk_part [total_chunks] scratch,
 *   norm_coef[0] = the global L2 norm of the gradients before clipping, norm_coef[1] = min(1, max_norm / (norm + 1e-6)), every gradient
 *   multiplied by it in place.  Nothing is read back by the host.
 * Activations (x, dy, dx, out, pred, a ...) are of dtype `dt` / `odt`: 0 = fp32, 1 = bf16 or 3 = fp16 storage with fp32 arithmetic and one
 *   rounding at the store; gains, targets and every sum (dyxr, part, loss, norm) are fp32.
 * vt_mse_loss: F.mse_loss and its gradient: loss[0] = mean((pred - target)^2), dpred = 2 (pred - target) / n.
 * vt_mse_loss_scaled (fp16 training with a loss scale): the same loss, NOT scaled, and dpred = grad_scale * 2 (pred - target) / n rounded once.
 * vt_grad_unscale_clip_multi: GradScaler.unscale_ followed by clip_grad_norm_ over the table whose gradients are inv_scale^-1 times too large:
 *   found_inf[0] = 1 if any RAW gradient element is inf or NaN, else 0 (cleared by this call, set by an integer atomic); norm_coef[0] = the
 *   L2 norm of g * inv_scale, norm_coef[1] = min(1, max_norm / (norm + 1e-6)); then, only if the flag is clear, g = (g * inv_scale) * coef as
 *   two multiplications (torch's bits for any scale).  With the flag set no gradient is written.  The float sums have a fixed order: two calls
 *   give the same bits.  The caller reads found_inf to decide whether the optimizer step is taken. */
typedef struct {
  const void *Q, *K, *V, *dO;
  void *dQ, *dK, *dV;
  float* ws;
  const unsigned char* kmask;
  long km_bs;
  long q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, v_bs, v_rs, v_hs, do_bs, do_rs, do_hs;
  long dq_bs, dq_rs, dq_hs, dk_bs, dk_rs, dk_hs, dv_bs, dv_rs, dv_hs;
  int B, H, Nq, Nk, hd, dtype;
  float scale;
} VtAttnBwdParams;
int vt_attention_bwd(const VtAttnBwdParams* params, vt_stream_t stream);
/* vt_attention_bwd_mfma (csrc/vt_attn_bwd.hip): the same gradients on 16-bit MFMA, for bf16 or fp16 operands (dtype 1 / 3; fp16 rounds P, dS and
 *   the results to fp16 instead, without clamping: tests/attn_bwd_mfma16_ref.py), head_dim 64, 1 <= Nq <= 128, any Nk >= 1.
 *   One rounding more than vt_attention_bwd: P and dS = P (dP - delta) are rounded to bf16 (nearest even) before they multiply dO, Q and K; the
 *   scale is applied to the fp32 sums afterwards (tests/attn_bwd_mfma_ref.py states the arithmetic).  Unit inner stride, every other stride a
 *   multiple of 8 elements, every base 16-byte aligned.  `ws` receives (max, 1 / sum, delta) as above; `ws2` (16-byte aligned, at least
 *   vt_attention_bwd_mfma_ws_bytes(B, H, Nq, Nk) bytes, which is < 0 for a shape this entry does not take) holds per-key-run partial results.
 *   Anything outside the contract is refused (VT_ERR_UNSUPPORTED / VT_ERR_ARG and a message) before any launch: there is no fallback.  No
 *   allocation, no synchronisation, no atomics: two calls give the same bits.  vt_attention_bwd stays the default of the trainer and the only
 *   fp32 path. */
long vt_attention_bwd_mfma_ws_bytes(int B, int H, int Nq, int Nk);
int vt_attention_bwd_mfma(const VtAttnBwdParams* params, void* ws2, long ws2_bytes, vt_stream_t stream);
int vt_rmsnorm_bwd(const void* x, const float* w, const void* dy, void* dx, float* dyxr, int rows, int D, float eps, int mode, int dt, vt_stream_t stream);
int vt_headnorm_bwd(const void* x, long x_stride, void* dy, long dy_stride, int heads, long tokens, const float* w, float* part, float eps,
                    int mode, int dt, vt_stream_t stream);
int vt_act_bwd(const void* x, const void* dy, void* out, long n, int act, int dt, vt_stream_t stream);
int vt_ddpm_qsample(const float* state, const float* action, const float* noise, const float* mask, const long* timesteps,
                    const float* alphas_cumprod, int num_train_timesteps, void* out, int odt, int B, int horizon, int action_dim, vt_stream_t stream);
int vt_timestep_embed(const float* t, const float* freqs, void* out, int odt, int B, int dim, vt_stream_t stream);
int vt_add_rowvec_(void* a, int dt, const float* v, long rows, long cols, vt_stream_t stream);
int vt_transpose_pad(const void* in, void* out, int dt, int M, int N, int Mp, vt_stream_t stream);
/* vt_colsum / vt_add_ / vt_copy_cols (fp32 only, above) for an activation dtype `dt` (0 fp32, 1 bf16, 3 fp16): column sums in fp32, a += b, dst[:, doff..] = src[:, off..] */
int vt_colsum_dt(const void* x, int dt, long ld, float* out, int M, int N, vt_stream_t stream);
int vt_add_dt(void* a, const void* b, long n, int dt, vt_stream_t stream);
/* vt_gemm_tn (csrc/vt_gemm_tn.hip): a Linear's weight gradient on 16-bit MFMA with no transposed copy of an operand:
 *   dw[N][K] = sum_m dy[m][n] x[m][k] (fp32, row pitch K) and, if db is not null, db[N] = sum_m dy[m][n] (fp32) from the same launch.
 *   dy [M][N] and x [M][K] are both bf16 or both fp16 (dt 1 / 3), rows token-major with unit inner stride and row pitches ld_dy >= N, ld_x >= K in
 *   elements, so a column slice of a wider buffer is read in place.  M >= 1 (int), N and K multiples of 8, pitches multiples of 8, every base
 *   16-byte aligned.  Products are exact and accumulated in fp32.  Anything else (fp32 operands included) is refused with VT_ERR_ARG and a
 *   message before any launch: there is no fallback.
 * vt_gemm_tn_plan: host only, a pure function of (M, N, K): the token rows are cut into `splits` runs of `rows_per_split` rows (a multiple of
 *   m_step = 32, the kernel's reduction step; the last run may be shorter), split s = rows s * rows_per_split ... of dy and x.  splits = 1:
 *   ws_bytes = 0, ws may be null and dw / db are stored directly.  splits > 1: ws (device, 16-byte aligned, at least ws_bytes =
 *   splits * (N * K + N) * 4 rounded up to a multiple of 256) receives per split an fp32 partial [N][K] followed by a db partial [N], and a
 *   second kernel adds them in split order.  The rule: splits = min(ceil(256 / tiles), floor(ceil(M / 32) / 4), 16), at least 1, for
 *   tiles = ceil(N / 128) * ceil(K / 128) workgroup tiles; rows_per_split = ceil(ceil(M / 32) / splits) * 32; splits = ceil(M / rows_per_split).
 *   No allocation, no synchronisation, no atomics, no counters: the bits depend on the shapes only, and two calls give the same bits.
 *   Returns VT_OK, or VT_ERR_ARG for M < 1 or an N or K that is not a positive multiple of 8 (the plan is then zeroed). */
typedef struct {
  int splits, rows_per_split, m_step;
  long ws_bytes;
} VtGemmTnPlan;
int vt_gemm_tn_plan(int M, int N, int K, VtGemmTnPlan* plan);
int vt_gemm_tn(const void* dy, long ld_dy, const void* x, long ld_x, int dt, int M, int N, int K, float* dw, float* db, void* ws, long ws_bytes, vt_stream_t stream);
int vt_copy_cols_dt(const void* src, long lds, long off, void* dst, long ldd, long doff, long rows, long cols, int dt, vt_stream_t stream);
/* vt_refresh16 (csrc/vt_refresh16.hip): the 16-bit trainer's weight refresh, one read of an fp32 master W [N][K] (row pitch ldw >= K elements)
 *   writing whichever of four 16-bit forms (dt 1 bf16 / 3 fp16) are not null, in one launch:
 *     w16  [N][K]   the bits of vt_cast(W) (round to nearest even),
 *     w16t [K][Np]  vt_transpose_pad(w16), Np = N rounded up to 8, padding columns zero,
 *     wp            vt_pack_w32(w16)  (N % 32 == 0 and K % 16 == 0),
 *     wtp           vt_pack_w32 of w16t viewed [K][Np]  (K % 32 == 0 and Np % 16 == 0).
 *   w16t, wp and wtp are 16-byte aligned; wp also wants a 16-byte aligned master and w16 and ldw % 4 == 0.  A null master, N or K below 1,
 *   ldw < K, another dtype or a packed form asked for a shape vt_pack_w32 refuses returns VT_ERR_ARG before any launch and writes nothing;
 *   an output that is null is never touched.  Stands where DeepSpeed's bf16 optimizer copies its fp32 partitions back into the 16-bit
 *   parameters after a step; the transposed and packed forms are layouts of this engine's GEMM tiles. */
int vt_refresh16(const float* W, long ldw, int N, int K, int dt, void* w16, void* w16t, void* wp, void* wtp, vt_stream_t stream);
int vt_grad_clip_multi(const void* table, int ntensors, long total_chunks, float max_norm, float* chunk_part, float* norm_coef, vt_stream_t stream);
int vt_mse_loss(const void* pred, const float* target, void* dpred, float* loss, long n, int dt, vt_stream_t stream);
int vt_mse_loss_scaled(const void* pred, const float* target, void* dpred, float* loss, long n, int dt, float grad_scale, vt_stream_t stream);
int vt_grad_unscale_clip_multi(const void* table, int ntensors, long total_chunks, float max_norm, float inv_scale, float* chunk_part, float* norm_coef,
                               int* found_inf, vt_stream_t stream);
/* Gradient accumulation over the table of vt_adamw_ema_multi, whose g column holds the persistent fp32 accumulators.
 * vt_grad_accum_multi: fresh = device array of ntensors `const float*`, the micro-batch's gradients in table order.  accumulate = 0:
 *   acc = g * scale (the accumulator is not read); otherwise acc = fma(g, scale, acc).  scale = 1 / gradient_accumulation_steps.
 * vt_ema_multi: the EMA half of vt_adamw_ema_multi alone (records without a shadow are skipped), 1 - decay read from hyper[3]: the bits of
 *   vt_ema_update_dev per tensor. */
int vt_grad_accum_multi(const void* table, const void* fresh, int ntensors, long total_chunks, float scale, int accumulate, vt_stream_t stream);
int vt_ema_multi(const void* table, int ntensors, long total_chunks, const float* hyper, vt_stream_t stream);
/* The bf16 gradient exchange of data-parallel fine-tuning.  comm_bf16: total_chunks * 4096 bf16 on the device, 16-byte aligned, laid out as
 * the table implies: tensor i occupies [first_chunk_i * 4096, first_chunk_i * 4096 + n_i), the rest of its last chunk is padding.
 * vt_grad_fold_pack_multi: the window's last fold and the rounding in one pass.  comm = bf16 (round to nearest even, any NaN as 0x7FC0) of the
 *   fp32 value vt_grad_accum_multi would have stored with the same arguments (g * scale, or fma(g, scale, acc)); the padding is written as
 *   zeros; the accumulators (the table's g column) are read when accumulate != 0 and never written.
 * vt_grad_unpack_multi: acc[e] = float(comm[first_chunk_i * 4096 + e]) for the n_i elements of every tensor; nothing else is written.
 * One 256-thread block per chunk, no atomics, no allocation: two calls give the same bits. */
int vt_grad_fold_pack_multi(const void* table, const void* fresh, int ntensors, long total_chunks, float scale, int accumulate, void* comm_bf16,
                            vt_stream_t stream);
int vt_grad_unpack_multi(const void* table, const void* comm_bf16, int ntensors, long total_chunks, vt_stream_t stream);
/* AdamW with block-wise 8-bit moments (csrc/vt_adam8.hip; the dynamic block-wise quantisation of Dettmers et al., "8-bit Optimizers via
 * Block-wise Quantization"; stands where the reference passes --use_8bit_adam, train/train.py:216-237; the arithmetic is stated in
 * DESIGN.md §8 and tests/adam8_ref.py, UNPINNED against bitsandbytes).  A moment tensor is n uint8 codes into a 256-entry table plus one
 * fp32 scale per block of 256 consecutive elements (the last block may be partial): value = T[code] * scale.
 * tables: 1024 fp32 on the device = T_s[256] (signed, first moment) | T_u[256] (unsigned, second moment) | B_s[256] | B_u[256], with
 *   B[j] = fp32(((double)T[j] + T[j+1]) / 2) for j < 255 and B[255] = +inf.  The code of x is the number of B[j] strictly below x: the nearest
 *   table value, ties to the lower index.  vlatouch/adam8.py builds the buffer.
 * vt_adamw8_ema_multi: one launch over the table of vt_adamw_ema_multi, whose m / v columns hold `unsigned char*` code pointers for the
 *   records that aux marks as quantised.  aux = ntensors records of 2 x 8 bytes {float* am, float* av} (ceil(n / 256) scales each); a null
 *   pair means fp32 m / v for that record, which is then updated with the bits of vt_adamw_ema_multi.  Per block: m = T_s[m8] am,
 *   v = T_u[v8] av; p, m', v' (and the shadow) as vt_adamw_ema_multi computes them, p from the unquantised m', v'; am' = max |m'|,
 *   av' = max v'; m8' = code_s(m' / am') (127 when am' = 0), v8' = code_u(v' / av') (0 when av' = 0).  No allocation, synchronisation or
 *   atomics: two calls on the same inputs give the same bits.
 * vt_adam8_quantize / vt_adam8_dequantize: the same block rule on its own; signed_table 1 = T_s with absmax = max |x|, 0 = T_u with
 *   absmax = max(x, 0); codes [n], absmax [ceil(n / 256)]. */
int vt_adamw8_ema_multi(const void* table, const void* aux, const float* tables, int ntensors, long total_chunks, const float* hyper, float beta1,
                        float beta2, float eps, float weight_decay, vt_stream_t stream);
int vt_adam8_quantize(const float* x, unsigned char* codes, float* absmax, const float* tables, int signed_table, long n, vt_stream_t stream);
int vt_adam8_dequantize(const unsigned char* codes, const float* absmax, const float* tables, int signed_table, float* out, long n, vt_stream_t stream);
/* Metrics of fine-tuning's periodic sampling evaluation (VLA/train/sample.py:55-86, log_sample_res), one call per evaluation batch.
 * pred [B][H][A] of dtype `dt` (0 fp32, 1 bf16, 3 fp16), target [B][H][A], mask [B][A] (0 / 1) and state_norm [B][A] fp32, the last two
 * broadcast over H; dataset_idx [B] int32 in [0, n_datasets).  Per element in fp32: sq = (pred - target)^2, l2 = sqrt(sq) / (state_norm + 1e-3).
 *   per_sample [B][2] = (sum sq m / sum m, sum l2 m / sum m) over the sample's H * A elements, overall [2] = the same two ratios over the whole
 *   batch; sums in fp64, rounded once at the fp32 store.  A sample whose mask is all zero gives NaN (0 / 0) and adds zero to the overall sums.
 *   Running state of one evaluation, zeroed by the caller before its first batch: acc [n_datasets + 1][2] fp64 and count [n_datasets + 1]
 *   int32.  Row dataset_idx[b] receives per_sample[b] (the fp32 values, in index order) and a count, row n_datasets the overall pair.
 *   ws: 3 * B doubles of scratch.  Two launches, no atomics (two calls give the same bits), no host read, allocation or synchronisation. */
int vt_sample_metrics(const void* pred, int dt, const float* target, const float* mask, const float* state_norm, const int* dataset_idx, int B,
                      int H, int A, int n_datasets, float* per_sample, float* overall, double* acc, int* count, double* ws, vt_stream_t stream);

/* ---- camera frames -> SigLIP pixel_values (scripts/franka_model_eef.py:242-288: RoboticDiffusionTransformerModel.preprocess_images + the
 * `.to(device, dtype)` of step(); SiglipImageProcessor.preprocess).  Bit-identical to that PIL path: optional brightness lift
 * (v' = min(255, (int)(1.75f * v)) when sum / (h * w * 255.0 * 3) <= 0.15, decided on the device), pad to a square with `fill_rgb` (never
 * materialised; the fill is not lifted), PIL's 8-bit antialiased resampler (horizontal pass, uint8 intermediate, vertical pass), then the
 * normalise table.  One frame = one record of the table below; the caller passes the table twice, as host memory (checked here, sizes the
 * launches) and as the same bytes in device memory (read by the kernels).
 * Coefficient table of one axis (device int32, built by the host in double for (in, out, filter); vlatouch/imgprep.py):
 *   [out][2] = (first input index, tap count), then [out][ksize] taps in 22-bit fixed point; a null table = the axis is already at its
 *   output size and the pass is skipped, as PIL skips it.
 * flags: VT_IMGPREP_PAD, VT_IMGPREP_BRIGHT, output VT_IMGPREP_OUT_BF16 (default fp32) -> out [n][3][S][S] through `lut` ([3][256] of the
 *   output dtype; out 16-byte aligned); VT_IMGPREP_OUT_U8 -> plain resample to uint8 HWC, frame i at out + out_off (the `image_size`
 *   pre-resize; no pad / brightness / missing frames, lut unused, S ignored); VT_IMGPREP_TWO_PASS forces the two-launch form.
 * A missing frame (src null) becomes the S x S image of fill_rgb.  fill_rgb = r | g << 8 | b << 16.
 * The fused kernel holds at most 128 intermediate rows per 16-row output tile (rows_max): calls with a larger frame, and the uint8 mode,
 * run horizontal and vertical passes as two launches through a uint8 scratch in `ws`.
 * vt_imgprep_workspace_bytes checks the table, WRITES every record's ws_off and returns the bytes vt_imgprep needs (0 on a bad table,
 * see vt_last_error); copy the table to the device after it. */
typedef struct {
  const void* src;      /* uint8 HWC RGB, device; null = missing frame */
  const void* coef_h;   /* coefficient table of the horizontal pass (input = padded width), or null */
  const void* coef_v;   /* ... of the vertical pass (input = padded height), or null */
  long pitch;           /* bytes between rows of src, >= 3 * w */
  int h, w;             /* frame size */
  int out_h, out_w;     /* output size (= S unless VT_IMGPREP_OUT_U8) */
  int ksize_h, ksize_v; /* taps per output index in the tables */
  int rows_max;         /* most input rows any 16-row output tile reads: max over y0 = 0, 16, .. of first[y1] + count[y1] - first[y0], y1 = min(y0 + 15, out_h - 1); 16 without a vertical table */
  int reserved;
  long out_off;         /* VT_IMGPREP_OUT_U8: byte offset of this frame's output */
  long ws_off;          /* written by vt_imgprep_workspace_bytes */
} vt_imgprep_frame;
#define VT_IMGPREP_PAD 1
#define VT_IMGPREP_BRIGHT 2
#define VT_IMGPREP_OUT_BF16 4
#define VT_IMGPREP_OUT_U8 8
#define VT_IMGPREP_TWO_PASS 16
size_t vt_imgprep_workspace_bytes(vt_imgprep_frame* frames_host, int n, int S, int flags);
int vt_imgprep(const vt_imgprep_frame* frames_host, const void* frames_dev, int n, int S, const void* lut, unsigned fill_rgb, int flags,
               void* out, void* ws, size_t ws_bytes, vt_stream_t stream);

/* ---- colour jitter of camera frames (train/dataset.py:379-391: the brightness lift and transforms.ColorJitter on PIL images, i.e.
 * PIL.ImageEnhance.Brightness / Contrast / Color and the HSV round trip of Image.convert).  Bit-identical to PIL; uint8 HWC RGB in, uint8
 * HWC RGB out.  Per frame up to four operations in a stated order:
 *   brightness(f) = blend(0, v, f);  saturation(f) = blend(L(pixel), v, f);  contrast(f) = blend(m, v, f) with
 *   m = (int)((double)sum of L / (double)(h * w) + 0.5) over the frame as the operations before contrast left it;
 *   hue(shift): RGB -> HSV, H = (H + shift) & 255, HSV -> RGB as Pillow's Convert.c;
 *   blend(a, b, f) = Image.blend per byte: t = (float)a + f * ((float)b - (float)a) in fp32 without contraction, 0 for t <= 0, 255 for
 *   t >= 255, else (int)t;  L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16.
 * order[k]: the operation of slot k (VT_COLORJITTER_BRIGHTNESS .. _HUE), VT_COLORJITTER_NONE skips the slot; no operation twice.  Any
 * subset in any order can be stated, the empty one included (the frame is then copied, or only lifted).
 * flags: VT_COLORJITTER_LIFT applies the brightness lift of vt_imgprep (v' = min(255, (int)(1.75f * v)) when sum / (h * w * 255.0 * 3) <= 0.15
 * on the frame as given, decided on the device) before the operations.
 * Two launches: exact integer sums (one uint64 partial per block in `ws`, every slot rewritten, no atomics; skipped when no frame needs
 * one), then the per-pixel pass.  Frame i is written tight (pitch 3 * w) at out + out_off; source and output must not overlap.
 * The table is passed as host memory (checked here) and as the same bytes in device memory (read by the kernels).  n < 1, a null source,
 * an unknown or repeated operation id and a short workspace return VT_ERR_ARG without a launch. */
typedef struct {
  const void* src;      /* uint8 HWC RGB, device */
  long pitch;           /* bytes between rows of src, >= 3 * w */
  int h, w;             /* frame size */
  long out_off;         /* byte offset of this frame's output in `out` */
  int order[4];         /* operation ids in application order */
  float brightness, contrast, saturation;   /* blend factors of the three enhance operations */
  unsigned char hue_shift;                  /* byte added to H (int(hue * 255) mod 256) */
  unsigned char reserved[3];
} vt_colorjitter_frame;
#define VT_COLORJITTER_BRIGHTNESS 0
#define VT_COLORJITTER_CONTRAST 1
#define VT_COLORJITTER_SATURATION 2
#define VT_COLORJITTER_HUE 3
#define VT_COLORJITTER_NONE 4
#define VT_COLORJITTER_LIFT 1
size_t vt_colorjitter_workspace_bytes(int n);
int vt_colorjitter(const vt_colorjitter_frame* frames_host, const void* frames_dev, int n, int flags, void* out, void* ws, size_t ws_bytes,
                   vt_stream_t stream);

/* ---- the pixel mapping of a JPEG round trip of camera frames (residual_controller/frank_inference_eef.py:84-87 and
 * data/create_controller_dataset_episode.py:54-62: cv2.imencode('.jpg') -> cv2.imdecode, "to align with training").  Bit-identical to
 * libjpeg with jpeg_set_defaults at `quality` (Annex K tables scaled as jpeg_set_quality does, 4:2:0, islow DCT) and a default decompress
 * (islow, fancy up-sampling; components at most 2 samples wide are replicated, as jdsample.c does); the entropy coder is lossless and is
 * not run.  uint8 HWC in (pitched), uint8 HWC out, frame i tight (pitch 3 * w) at out + out_off; source and output must not overlap.
 * flags: VT_JPEGMAP_CV2_ORDER: channel 0 of the array plays blue's role, as cv2 treats whatever it is given; without it channel 0 is red.
 * Two launches: per 16 x 16 MCU the conversion, down-sampling, forward DCT, quantise / dequantise and inverse DCT into the decoded planes
 * Y' | Cb' | Cr' in `ws` (1.5 bytes per pixel of the frame padded to multiples of 16), then per output pixel the up-sampling and the
 * conversion back.  int32 arithmetic, no atomics: a pure function of the inputs.  No host read, allocation or synchronisation.
 * vt_jpegmap_workspace_bytes checks the table, WRITES every record's ws_off and returns the bytes vt_jpegmap needs (0 on a bad table, see
 * vt_last_error); copy the table to the device after it.  The table is passed as host memory (checked here) and as the same bytes in device
 * memory (read by the kernels).  n < 1, a null source, h < 1, w < 1, a side above 32768, pitch < 3 * w, quality outside 1..100, unknown flag
 * bits, a ws_off that vt_jpegmap_workspace_bytes did not write and a short or misaligned (8 bytes) workspace return VT_ERR_ARG without a
 * launch. */
typedef struct {
  const void* src;      /* uint8 HWC, device */
  long pitch;           /* bytes between rows of src, >= 3 * w */
  int h, w;             /* frame size */
  long out_off;         /* byte offset of this frame's output in `out` */
  long ws_off;          /* written by vt_jpegmap_workspace_bytes */
} vt_jpegmap_frame;
#define VT_JPEGMAP_CV2_ORDER 1
size_t vt_jpegmap_workspace_bytes(vt_jpegmap_frame* frames_host, int n);
int vt_jpegmap(const vt_jpegmap_frame* frames_host, const void* frames_dev, int n, int quality, int flags, void* out, void* ws,
               size_t ws_bytes, vt_stream_t stream);

/* ---- baseline JPEG files decoded on the device (vlatouch/jpegdec.py; csrc/vt_jpegdec.hip), bit-identical to libjpeg's default decompress
 * (islow inverse DCT, fancy h2v2 up-sampling, components at most 2 samples wide replicated): three components, 4:2:0 or 4:4:4, one
 * interleaved scan.  The host parses the markers, un-stuffs FF 00 and removes the RSTn markers; the Huffman decoder, the dequantisation, the
 * inverse DCT, the up-sampling and the conversion run here.  Output: uint8 HWC, frame i tight (pitch 3 * w) at out + out_off.
 * A table is int64 [n][VT_JPEG_K], passed as host memory (checked here) and as the same bytes in device memory (read by the kernels).  A row:
 *    0 stream     device pointer, 4-byte aligned: the un-stuffed entropy bytes, padded with FF to a multiple of 4
 *    1 len        bytes of the stream before the padding (< 2^28)
 *    2 h   3 w    frame size (1..32768)
 *    4 sampling   VT_JPEG_444 or VT_JPEG_420
 *    5 tables     device pointer, 4-byte aligned: a table set of VT_JPEG_TABLESET_BYTES (layout: csrc/vt_jpegdec.hip)
 *    6 entries    device pointer, 16-byte aligned: int32 [ceil(mcus / interval)][4] = bit offset, DC predictors of Y, Cb, Cr
 *    7 interval   MCUs per entry (1..mcus)
 *    8 restart    the restart interval in MCUs, 0 = none
 *    9 starts     device pointer, 4-byte aligned: int32 byte offset in the stream of every restart interval's start ([0] = 0)
 *   10 out_off    byte offset of this frame's output in `out` (vt_jpeg_decode)
 *   11 12         workspace offsets, WRITTEN by vt_jpeg_workspace_bytes, which returns the bytes vt_jpeg_decode needs (0 on a bad table)
 *   13..15        reserved, 0
 * vt_jpeg_index (once per upload) walks every stream, one lane per restart interval, and writes the entries.  vt_jpeg_decode decodes the n
 * frames of the table: one lane per entry Huffman-decodes `interval` MCUs into int16 coefficients in the workspace; then dequantise +
 * inverse DCT into decoded planes; then up-sampling and conversion.  status: int32 [n] on the device, zeroed by the caller; a lane that
 * meets an undefined code, a run past coefficient 63 or the end of the stream before its MCUs are done stores 1 in its frame's word and
 * zero-fills the rest of its MCUs.  Stream reads are clamped to the padded length (1-bits behind it, as libjpeg pads).  No atomics: a pure
 * function of the inputs.  No host read, allocation or synchronisation.  A bad row (sizes, sampling code, null or misaligned pointers,
 * interval, workspace offsets not the ones written), n < 1, a null buffer and a short or misaligned (16 bytes) workspace return
 * VT_ERR_ARG without a launch. */
#define VT_JPEG_K 16
#define VT_JPEG_444 0
#define VT_JPEG_420 1
#define VT_JPEG_TABLESET_BYTES 6144
size_t vt_jpeg_workspace_bytes(long long* table_host, int n);
int vt_jpeg_index(const long long* table_host, const void* table_dev, int n, void* status, vt_stream_t stream);
int vt_jpeg_decode(const long long* table_host, const void* table_dev, int n, void* out, void* ws, size_t ws_bytes, void* status,
                   vt_stream_t stream);

/* ---- corruption of camera frames (train/image_corrupt.py: imgaug's Sequential([noise, blur], random_order=True)), restated in integers
 * (UNPINNED against imgaug and cv2).  uint8 HWC in (pitched), uint8 HWC out, frame i tight (pitch 3 * w) at
 * out + out_off; source and output must not overlap.  Per frame, in the stated order, either or both of
 *   noise: v' = clamp(v + e, 0, 255), e = -255 + #{n in -255..254 : u >= C[n]} with C the frame's VT_CORRUPT_THRESHOLDS non-decreasing
 *     thresholds (C[n] = floor(2^32 P(X <= n)), built by the host) and u = word idx & 3 of Philox4x32-10 at counter idx >> 2 under `key`;
 *     idx = (y * w + x) * 3 + c with per_channel, y * w + x (one draw for the three bytes) without.  Behind a blur, (y, x) is the output
 *     position; in front of it, the position of the source pixel, so a pixel reached through the border carries its own noise;
 *   blur: GAUSSIAN, AVERAGE, MOTION: ntaps taps (dy, dx, W > 0) as int32 triples, |dy|, |dx| <= k / 2 <= VT_CORRUPT_MAX_RADIUS, tap_sum = D
 *     = sum of W <= 2^24; per byte S = sum of W * p(y + dy, x + dx) over the periodic reflect-101 border (period 2 (n - 1); n = 1 reads
 *     index 0), q, r = divmod(S, D), out = q + (2 r > D or (2 r == D and q odd)).  k: odd in 3..37, for AVERAGE 2..7.
 *     MEDIAN: per channel the median of the k x k window over the replicate border, k odd in 3..11, exact.
 * The thresholds and taps of all frames sit in one buffer of 32-bit words at noise_off / taps_off (in words); like the frame table it is
 * passed as host memory (checked here) and as the same bytes in device memory (read by the kernel).
 * One launch: a workgroup stages a 32 x 32 tile plus halo in LDS, blurs out of LDS, writes words.  No workspace, no atomics, no host read,
 * allocation or synchronisation: a pure function of the inputs.  n < 1, a null source, h < 1, w < 1, pitch < 3 * w, an unknown kind or
 * order, an even or out-of-range k, decreasing thresholds, an empty tap list, a tap beyond radius k / 2, a weight < 1, tap_sum that is not
 * the taps' sum or lies outside 1..2^24, and a table that does not hold what a record points at return VT_ERR_ARG without a launch. */
typedef struct {
  const void* src;      /* uint8 HWC, device */
  long pitch;           /* bytes between rows of src, >= 3 * w */
  int h, w;             /* frame size */
  long out_off;         /* byte offset of this frame's output in `out` */
  unsigned long long key;   /* Philox key of the frame's noise */
  int noise;            /* VT_CORRUPT_NOISE_*: which distribution the thresholds state (the device reads them only) */
  int per_channel;      /* 0: one draw per pixel, shared by its three bytes */
  int blur, k;          /* VT_CORRUPT_BLUR_*, and the kernel's side */
  int order;            /* VT_CORRUPT_NOISE_FIRST / VT_CORRUPT_BLUR_FIRST */
  int noise_off;        /* word offset of C[510] in the tables */
  int taps_off, ntaps;  /* word offset of the int32 (dy, dx, W) triples, and their count */
  unsigned tap_sum;     /* D */
  unsigned reserved;
} vt_corrupt_frame;
#define VT_CORRUPT_NOISE_NONE 0
#define VT_CORRUPT_NOISE_GAUSSIAN 1
#define VT_CORRUPT_NOISE_LAPLACE 2
#define VT_CORRUPT_NOISE_POISSON 3
#define VT_CORRUPT_BLUR_NONE 0
#define VT_CORRUPT_BLUR_GAUSSIAN 1
#define VT_CORRUPT_BLUR_AVERAGE 2
#define VT_CORRUPT_BLUR_MEDIAN 3
#define VT_CORRUPT_BLUR_MOTION 4
#define VT_CORRUPT_NOISE_FIRST 0
#define VT_CORRUPT_BLUR_FIRST 1
#define VT_CORRUPT_THRESHOLDS 510
#define VT_CORRUPT_MAX_RADIUS 18
#define VT_CORRUPT_MAX_TAP_SUM (1u << 24)
int vt_corrupt(const vt_corrupt_frame* frames_host, const void* frames_dev, int n, const unsigned* tables_host, const void* tables_dev,
               long table_words, void* out, vt_stream_t stream);

/* ---- the reference's zero pad and area resize of camera frames (scripts/utils_eef.py:5-77, pad_and_resize_for_siglip: the frame centred
 * on a zero square of side m = max(h, w), rows from (m - h) / 2 and columns from (m - w) / 2, both floored, then cv2.resize to
 * (target, target) with INTER_AREA), restated from OpenCV 4.x modules/imgproc/src/resize.cpp (UNPINNED against cv2).
 * uint8 HWC in (pitched), uint8 HWC out, frame i tight (pitch 3 * target) at out + out_off; source and output must not overlap.
 * In fp64, inv = (double)target / m, scale = 1.0 / inv, iscale = (int)scale:
 *   scale < 1 (a frame smaller than the target): cv2's fixed-point bilinear emulation, not built, refused;
 *   |scale - iscale| < DBL_EPSILON (resizeAreaFast_): ntaps = 0.  s = the integer sum of the iscale x iscale cell; iscale 1 copies, iscale
 *     2 gives (s + 2) >> 2, any other (float)s * (1.0f / (iscale * iscale)) rounded to nearest-even and clamped to 0..255;
 *   otherwise (resizeArea_<uchar, float>): ntaps >= 1 and the axis table at tabs + tab_x (columns) and tabs + tab_y (rows), device memory
 *     the host filled: [ntaps][target] pairs {int32 source index, fp32 weight} as computeResizeAreaTab lists them per output, the shorter
 *     lists padded with zero weights.  Per vertical tap (sy, beta) in order: buf = 0, then buf += (float)S[sy][sx] * alpha over the
 *     horizontal taps in order; sum = beta * buf for the first vertical tap, sum += beta * buf for the others; the output is sum rounded
 *     to nearest-even and clamped.  Every product and every sum is rounded to fp32 on its own (no fused multiply-add).
 * One launch over all frames, one output pixel per lane; the padded square is not made: a source position is clamped into the m x m
 * canvas and reads 0 in the border, so no table content can make a lane read outside its frame.  A pure function of the inputs.  No host
 * read, allocation or synchronisation.  n < 1, a null source, h < 1, w < 1, a side above 32768, pitch < 3 * w, target < 1, a frame
 * smaller than the target, ntaps that does not fit the form (0 for an integer scale, 1 .. iscale + 3 otherwise), an integer scale above
 * VT_AREA_MAX_ISCALE and a table offset that is negative, not a multiple of 8 or beyond tabs_bytes return VT_ERR_ARG without a launch. */
typedef struct {
  const void* src;      /* uint8 HWC, device */
  long pitch;           /* bytes between rows of src, >= 3 * w */
  int h, w;             /* frame size */
  long out_off;         /* byte offset of this frame's target x target output in `out` */
  int target;           /* output side */
  int ntaps;            /* taps per output of the axis tables; 0: the integer-scale form */
  long tab_x, tab_y;    /* byte offsets of the column and row tables in `tabs` (unused with ntaps = 0) */
} vt_area_frame;
#define VT_AREA_MAX_ISCALE 2048     /* 2048 * 2048 * 255 < 2^31 */
int vt_area_resize(const vt_area_frame* frames_host, const void* frames_dev, int n, void* out, const void* tabs, size_t tabs_bytes,
                   vt_stream_t stream);

/* ---- one fine-tuning micro-batch out of device-resident episodes (vlatouch/rdt_data.py).  Stands for, per sample,
 * UnifiedVLADataset.parse_file (data/unified_vla_dataset_episode.py:314-351: state row, action chunk from action_id = step_id + 2 padded
 * with its last row, the episode's std / norm, fill_in_state), VLAConsumerDataset.__getitem__ (train/dataset.py:327-344: control frequency,
 * state noise, the state / element-mask condition masks) and DataCollatorForVLAConsumerDataset (train/dataset.py:502-530: the stacks, the
 * zero-padded language embeddings and their mask).  The random draws are the host's; they arrive in `plan`.
 * Device-resident tables: qpos fp64 [sum N][S] with ep_off int32 [E + 1] (row offsets); ep_stats fp64 [E][3][S] = per-episode std | mean |
 *   rms; ds_mean fp64 [S], the dataset mean a masked state is replaced with; col_map int32 [A], unified column -> robot column or -1 (the
 *   inverse of the fill_in_state indices); lang fp32 [sum L][D] with lang_off int32 [E + 1].
 * plan (device, 8-byte aligned, one upload): int32 [B][4] = (episode, step_id, flags, 0) followed by fp64 z [B][S], the standard-normal
 *   draws of the state noise (read only for samples with VT_RDT_NOISE).
 * Outputs: states [B][1][A], actions [B][H][A], elem_mask [B][A], state_norm [B][A] fp32; ctrl_freqs [B] int64 (ctrl_freq, or 0 with
 *   VT_RDT_MASK_FREQ); lang_out [B][Lmax][D] fp32 and lang_mask [B][Lmax] bytes (1 = a token of the instruction).
 *   action row r = qpos[min(step_id + 2 + r, N - 1)]; state = qpos[step_id], with VT_RDT_NOISE + (0 + (std / noise_div) * z) in fp64
 *   without contraction (noise_div = sqrt(10^(snr / 10))), with VT_RDT_MASK_STATE ds_mean instead; elem_mask = 1 on the mapped columns, all
 *   zero with VT_RDT_MASK_ELEM; state_norm = the episode's rms; unmapped columns are 0.  Values are rounded to fp32 once, at the store.
 * Two launches, no atomics (two calls give the same bits), no host read, allocation or synchronisation.  The caller checks the plan against
 * its tables; an episode outside [0, E) is written as NaN rows and a step is clamped into its episode, so no entry reads outside the tables.
 * Null pointers, sizes < 1, A < S, a grid dimension above 65535, noise_div <= 0 and a misaligned plan return VT_ERR_ARG without a launch. */
#define VT_RDT_MASK_FREQ 1
#define VT_RDT_MASK_STATE 2
#define VT_RDT_MASK_ELEM 4
#define VT_RDT_NOISE 8
int vt_rdt_batch(const double* qpos, const int* ep_off, const double* ep_stats, const double* ds_mean, const int* col_map, const float* lang,
                 const int* lang_off, int E, int S, int A, int H, int D, int Lmax, int ctrl_freq, double noise_div, const void* plan, int B,
                 float* states, float* actions, float* elem_mask, float* state_norm, long long* ctrl_freqs, float* lang_out,
                 unsigned char* lang_mask, vt_stream_t stream);

/* ---- one controller-training batch out of device-resident episodes (vlatouch/ctrl_data.py).  Stands for, per sample,
 * ControllerDataset.__getitem__ (controller_dataset.py:101-170: the window's pose rows, VLA chunk and force rows), normalize_actions
 * (:303-346), the slicing of DiffusionControllerTrainer._prepare_batch_for_diffusion (bridge_train.py:105-164) or
 * LSTMControllerTrainer._prepare_batch (lstm_train.py:56-84) and the concatenation in front of the observation MLP; and, per step, for the
 * frozen DINOv2 tower, whose CLS vectors were encoded once per frame.
 * Device-resident tables: pose10 fp64 [rows][10] = converted_ee_pose_with_gripper, gripper NOT divided; vla fp64 [rows][Hv][10], the raw
 *   vla_action; forces fp32 [rows][Fd]; ep_off int32 [E + 1] (row offsets, rows = ep_off[E]); feat fp32 [2 cameras][rows][2 modes][dv], the
 *   CLS vector of each frame with the ImageNet normalisation off (mode 0) and on (mode 1); pix_sum uint64 [2][rows], the exact sum of each
 *   frame's P bytes (vt_ctrl_pixsum); stats fp32 [4][10] = expert mins | expert maxs | vla mins | vla maxs.
 * plan (device, one upload): int32 [B][2] = (episode, start).  The window's last context frame is f = start + cf - 1.
 * Normalisation decision, per camera, over the call's batch as the reference's DINOv2Encoder.forward takes it (visual_encoder.py:78,100):
 *   norm_flags[cam] = 1 iff 2 * sum_b pix_sum[cam][f_b] >= 255 * B * P, in exact integer arithmetic.  It replaces the fp32 mean of
 *   vt_dino_forward's statistics kernel and can differ from it only when the batch mean is within fp32 rounding of 0.5.
 * Outputs, fp32: obs_in [B][in_pad] = [feat[0][f][flag 0] | feat[1][f][flag 1] | pose10[f] | forces[f] | 0 ..] in vt_concat_obs's columns
 *   (the force columns only with VT_CTRL_BRIDGE and use_force); expert_act [B][h][10] = pose10[f + 1 + r] and vla_act [B][h][10] =
 *   vla[f + 1][r], gripper / 255 in fp64, rounded once to fp32, then normalised with the arithmetic of vt_action_normalize
 *   (padding_factor, the fp32 mins / maxs of `stats`); forces_out [B][h][Fd] = rows f + 1 .. f + h (VT_CTRL_BRIDGE) or f .. f + h - 1
 *   (VT_CTRL_LSTM, the reference's forces[:, cf - 1:-1]); current_force [B][Fd] = forces[f] (required for VT_CTRL_BRIDGE, may be null for
 *   VT_CTRL_LSTM); norm_flags [2].
 * Two launches, no atomics (two calls give the same bits), no host read, allocation or synchronisation.  The caller checks the plan against
 * its tables; an episode outside [0, E) or shorter than cf + h is written as NaN rows and adds nothing to the decision's sums, and a start
 * is clamped into [0, N - cf - h], so no entry reads outside the tables.  Null pointers, sizes < 1, h > Hv, an unknown layout, in_pad
 * smaller than the row, B, h or cf above 2^20, P above 2^32 and pose10 / vla not 16-byte aligned return VT_ERR_ARG without a launch. */
#define VT_CTRL_BRIDGE 0
#define VT_CTRL_LSTM 1
int vt_ctrl_batch(const double* pose10, const double* vla, const float* forces, const int* ep_off, const float* feat, const unsigned long long* pix_sum,
                  int E, long long rows, int Hv, int Fd, int dv, long long P, const float* stats, float padding_factor, int cf, int h, int layout,
                  int use_force, const int* plan, int B, float* obs_in, int in_pad, float* expert_act, float* vla_act, float* forces_out,
                  float* current_force, float* norm_flags, vt_stream_t stream);
/* sums [n] = the exact sum of the P bytes of each of n frames laid one after the other (uint8, any layout): what the decision above reads.
 * One block per frame, no atomics. */
int vt_ctrl_pixsum(const unsigned char* frames, long long P, int n, unsigned long long* sums, vt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
