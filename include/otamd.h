/* otamd.h -- C ABI of libotamd.so, the MI355X (gfx950) kernels of onetrainer_amd.
 *
 * Drop-in boundary for the diffusion train step of OneTrainer (modules/trainer/GenericTrainer.py:672-749
 * calling modules/modelSetup/<Family>Setup.predict / calculate_loss, loss.backward(), clip_grad_norm_,
 * optimizer.step()).  The reference is pure Python over diffusers/torch, so every entry point
 * below replaces an op the reference reaches through those libraries; each cites it.
 *
 * Conventions (all launchers):
 *   - plain device pointers, sizes and strides (in ELEMENTS), bf16 passed as void* (uint16 bits);
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream in the Python host);
 *   - no implicit allocation: scratch comes in through explicit workspace pointers;
 *   - return 0 on success, 1 = contract violated (shape / alignment; nothing launched),
 *     2 = launch error, 3 = unsupported configuration.  Python maps non-zero to RuntimeError;
 *   - thread-compatible; no global mutable state besides per-process tile-choice caching.
 * Layouts: activations NHWC (pixels x channels) / token-major [B, N, C]; conv weights
 * [Cout][kh][kw][Cin]; Linear weights [out][in]; attention Q/K/V/O [B, N, H*D] with strides.
 */
#ifndef OTAMD_H
#define OTAMD_H
#include <hip/hip_runtime.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { OTAMD_OK = 0, OTAMD_EINVAL = 1, OTAMD_ELAUNCH = 2, OTAMD_EUNSUPPORTED = 3 };

/* GEMM operand modes */
enum { OPM_K = 0, OPM_MN = 1, OPM_CONV_FWD = 2, OPM_CONV_DGRAD = 3, OPM_CONV_WGRAD = 4 };

typedef struct ConvGeom {
  int N, SH, SW, SC, RH, RW, KH, KW, stride, pad, upsample, pad_;
  long long ld;
} ConvGeom;

/* C[M,N] = alpha * op(A) op(B) (+bias[n]) (+rowvec[m/rows_per_vec][n]) (+residual[m][n]) (+C if accumulate) */
typedef struct GemmArgs {
  const void* A; long long lda; int amode;
  const void* B; long long ldb; int bmode;
  void* C; long long ldc; int c_f32; int accumulate;
  int M, N, K;
  float alpha;
  const void* bias;
  const void* rowvec; long long ldv; int rows_per_vec;
  const void* residual; long long ldr;
  float* slab;
  int k_per_split;
  ConvGeom ga, gb;
  /* optional second K segment [K1, K1+K2): A2 K-mode, B2 K-mode (or MN-mode when B is); LoRA up/down fused
     into the base GEMM (replaces the extra GEMM + add of LoRAModule.forward, modules/module/LoRAModule.py:318-322) */
  const void* A2; long long lda2;
  const void* B2; long long ldb2;
  int K1, K2;
  /* batched GEMM (K/MN modes, one segment, no split-K): grid.y = z < batch; operand bases move by
     (z / bdiv) * s0 + (z % bdiv) * s1 elements ((image, head) pairs of [B, N, H*D] activations) */
  int batch, bdiv;
  long long sa0, sa1, sb0, sb1, sc0, sc1;
  /* optional column sums of an MN-mode A over the K range (the bias gradient of a Linear / conv weight
     gradient dW = dY^T X: colsum[m] = sum_k dY[k][m], replaces the separate dY.sum(0) of autograd):
     bf16 or fp32 [M], overwritten or accumulated; with split-K the partials go to the workspace after the
     GEMM slabs (splits * M floats) and the split-K reduce folds them */
  void* colsum; int colsum_f32; int colsum_acc;
  float* colsum_slab;
  /* optional LoRA down-projection fused into a forward base GEMM (linear or 3x3 conv, B = K-mode weights, split 1,
     tiles 1 / 4 / 7 / 8, lora_r = 32): t = A D^T over the K loop for the adapter part of the tile's columns,
     rounded to bf16, stored to T [M][ldt] by the part's first tile column, and t (B2)^T added as the second K
     segment -- replaces the separate down GEMM x A^T + its split-K reduce before the fused up projection
     (LoRAModule.forward, modules/module/LoRAModule.py:318-322).  D = down [P*lora_r][K], B2 / ldb2 = up [N][P*lora_r],
     lora_pw = output columns per part; K = the base K, A2 = NULL.  D == NULL: off.
     The same fields on a linear input-gradient GEMM (A = dY K-mode, B = W MN-mode): u = dY (sB) for one adapter part
     spanning N (lora_pw = N), D = (sB)^T [lora_r][K], B2 / ldb2 = A^T [N][lora_r], T = u [M][ldt] -- the LoRA
     backward's dX = dY W + u A (LoRAModule.py:318-322 differentiated) without the separate u GEMM and its reduce. */
  const void* D; long long ldd;
  void* T; long long ldt;
  int lora_r, lora_pw;
} GemmArgs;

typedef struct AttnArgs {
  const void *q, *k, *v; void* o; float* lse;
  const void* dout; const float* delta; void *dq, *dk, *dv; float *dk32, *dv32;
  long long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  long long bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;
  int B, H, Nq, Nk, Dv;
  float scale;
  int qsplit, pad_;
} AttnArgs;

/* FLUX q/k RMSNorm + rotary embedding over 128-wide heads (csrc/flux.hip) */
typedef struct QKRopeArgs {
  const void* x; long long ldx; int qoff, koff;
  void* y; long long ldy; int yqoff, ykoff;
  const void* dy; long long lddy; int dyqoff, dykoff;
  const void *wq, *wk, *wq_ctx, *wk_ctx;
  const float *cs, *sn;
  float* dw_part;
  int rows, B, H, L;
  float eps;
  int pad_;
} QKRopeArgs;

typedef struct AdamwGroup {
  long long begin, end;
  float wd_factor, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, neg_step_size, pad;
} AdamwGroup;

typedef struct NormChunk { long long begin, end; int tensor, pad; } NormChunk;

/* Adafactor tables (csrc/adafactor.hip describes the modes and the slab layout) */
typedef struct AdafactorTensor {
  long long offset, numel;
  long long row_off, col_off, full_off;
  long long rpart_off, cpart_off, rmean_off;
  int batch, rows, cols, mode, group, slab_rows, row_slabs, col_tiles, slab0, n_slabs, pad0, pad1;
} AdafactorTensor;
typedef struct AdafactorSlab { long long row0, row1; int tensor, col0, col1, pad; } AdafactorSlab;
typedef struct AdafactorGroup {
  float lr, neg_wd, alpha_wd, eps1, eps2, clip_threshold, beta2t, one_minus_beta2t;
  int scale_parameter, pad;
} AdafactorGroup;

/* CAME (csrc/came.hip): the Adafactor tables above plus a fold table.  CameFold: kind 0 the global rows
   [i0, i1), kind 1 the global columns [i0, i1) of a mode 2 tensor (at most 256, a thread each), kind 2 the
   matrix i0 whose row-state mean is due */
typedef struct CameGroup {
  float lr, alpha_wd, eps1, eps2, clip_threshold;
  float beta1, one_minus_beta1, beta2, one_minus_beta2, beta3, one_minus_beta3;
  int pad;
} CameGroup;
typedef struct CameFold { long long i0, i1; int tensor, kind; } CameFold;

/* Prodigy (csrc/prodigy.hip).  ProdigyState: the device-resident scalars of the step size, all fp64; the host writes
   them at start-up and on load only.  dlr: d lr bc of the step in flight (from d before it); k: completed steps;
   skip: 1 when the step in flight found d_denom == 0.  ProdigyHyper: the launch arguments, passed by pointer from
   the host and by value to the kernels; beta3 resolved (sqrt(beta2) when the configuration leaves it open). */
typedef struct ProdigyState { double d, d_max, d_numerator, d_denom, d_hat, dlr, k, skip; } ProdigyState;
typedef struct ProdigyHyper {
  double lr, beta1, beta2, beta3, eps, weight_decay, d0, d_coef, growth_rate;
  int decouple, use_bias_correction, safeguard_warmup, pad;
} ProdigyHyper;

/* Schedule-free AdamW (csrc/schedule_free.hip).  SfGroup: one parameter group of a step, by value from the host:
   element range [begin, end) (begin a multiple of 8), lr after the warm-up factor, a_y = lr (beta1 (1 - ckp1) - 1),
   ckp1 = weight / weight_sum, beta2, 1 - beta2, 1 / bc2, eps, weight_decay; first: the group's first step (z = y is
   taken from the parameters instead of read).  SfSwapGroup: one group of a mode switch, p += w (z - p). */
typedef struct SfGroup {
  long long begin, end;
  float lr, a_y, ckp1, beta2, one_minus_beta2, inv_bc2, eps, weight_decay;
  int first, pad;
} SfGroup;
typedef struct SfSwapGroup { long long begin, end; float w; int pad; } SfSwapGroup;

/* 8-bit AdamW (csrc/adamw8bit.hip).  A8Seg: one tensor of the store, a host-built table sorted by begin: element range
   [begin, end) (begin a multiple of 8), blk0 its first 256-element work block (numbered consecutively through the
   table), state_off its first absmax entry (is8bit) or its first element in the fp32 side buffers (a multiple of 8),
   group the index of its A8Group.  A8Group: the scalars of one parameter group, by value from the host: beta1,
   1 - beta1, beta2, 1 - beta2, eps_c = sqrt(bc2) eps, step_size = -lr sqrt(bc2) / bc1, wd_factor = 1 - lr wd. */
typedef struct A8Seg {
  long long begin, end, blk0, state_off;
  int is8bit, group;
} A8Seg;
typedef struct A8Group {
  float beta1, one_minus_beta1, beta2, one_minus_beta2, eps_c, step_size, wd_factor, pad;
} A8Group;

/* replaces: diffusers Linear/Conv2d fwd+bwd inside model.unet(...) (modules/modelSetup/BaseStableDiffusionXLSetup.py:268-273); conv/linear dgrad/wgrad of loss.backward() (modules/trainer/GenericTrainer.py:693-696) */
int otamd_gemm(const GemmArgs* in, int splits, void* workspace, long long ws_bytes, hipStream_t stream);

/* plan query: workspace bytes otamd_gemm needs for `splits` (0 = automatic tile + split-K plan) */
long long otamd_gemm_plan(const GemmArgs* in, int splits, int* splits_out);

/* replaces: (plan override) the same GEMM with an explicit plan -- the autotuner's candidates and its
   cached per-shape choice (kernels.py set_gemm_autotune) and what otamd_gemm_resolve returns.  tile: a code of the
   tile catalogue (csrc/gemm_tiles.h lists them; -1 is the v1 128x128 kernel); splits >= 1;
   workspace >= splits*M*N*4 bytes when splits > 1 */
int otamd_gemm_explicit(const GemmArgs* in, int tile, int splits, void* workspace, long long ws_bytes,
                        hipStream_t stream);

/* replaces: (diagnostic) the tile the analytic planner gives these arguments and splits (0 = automatic) */
int otamd_gemm_plan_tile(const GemmArgs* in, int splits);
/* workspace bytes of a `splits`-way split-K launch (fp32 slabs, + the column-sum partials when colsum is set) */
long long otamd_gemm_ws_bytes(const GemmArgs* in, int splits);
/* BM x BN of a tile code; OTAMD_EINVAL for a code outside the catalogue */
int otamd_gemm_tile_dims(int tile, int* bm, int* bn);

/* Plan resolution (csrc/gemm_plan.hip; host code, no GPU needed).  The measured tables are data the Python package
   loads (gemm_plans_mi355x.json, lora_plans_mi355x.json) and stores here once per process; setting a table replaces
   it (exclusive lock), every lookup takes a shared lock.
   otamd_gemm_plan_key: the 16-field signature a measured plan is keyed by.
   otamd_gemm_set_plan_table: n rows of 18 = key, tile, splits.  otamd_gemm_plan_table_size: rows loaded.
   otamd_lora_set_plans: n rows of 6 = form, N, K, parts, M class (or -M: that exact row count), tile (-1: two launches).
   otamd_gemm_resolve: the (tile, splits) to launch with otamd_gemm_explicit; returns its workspace bytes (< 0: invalid
     arguments).  splits == 0: the measured plan, else the analytic one; splits > 0: the analytic tile for them.
   otamd_lora_plan: the fused-LoRA table's tile for a site (form 0 forward / 1 input gradient, base N and K, adapter
     parts, M rows): an exact-M entry first, then the class entry while its tile grid fills its rounds of CUs;
     0 = no entry or refused, -1 = two launches.
   otamd_lora_fused_tile: the tile a LoRA site launches fused on, 0 = two launches; `two_launch_base` is the base GEMM
     of the two-launch form (second K segment attached). */
int otamd_gemm_plan_key(const GemmArgs* in, long long key[16]);
int otamd_gemm_set_plan_table(const long long* rows, int n);
int otamd_gemm_plan_table_size(void);
int otamd_lora_set_plans(const long long* rows, int n);
long long otamd_gemm_resolve(const GemmArgs* in, int splits, int* tile, int* splits_out);
int otamd_lora_plan(int form, int N, int K, int parts, int M);
int otamd_lora_fused_tile(const GemmArgs* two_launch_base, int form, int parts);

/* replaces: ABI check */
int otamd_gemm_args_size(void);

/* replaces: ABI check */
int otamd_conv_geom_size(void);

/* replaces: F.scaled_dot_product_attention in diffusers Attention (attn1/attn2 of every BasicTransformerBlock) */
int otamd_attn_fwd(const AttnArgs* in, hipStream_t stream);

/* replaces: autograd of scaled_dot_product_attention (GenericTrainer.py:693-696) */
int otamd_attn_bwd(const AttnArgs* in, float* ws, long long ws_bytes, hipStream_t stream);

/* workspace bytes otamd_attn_bwd needs for these arguments (16-byte bias records per query + split-query or
   per-chunk dK/dV partials) */
long long otamd_attn_bwd_ws_bytes(const AttnArgs* in);

/* bytes of the fp32 dK / dV partial slabs alone (0: none needed), the caller-owned buffer of otamd_attn_bwd_ex */
long long otamd_attn_bwd_slab_bytes(const AttnArgs* in);

/* replaces: as otamd_attn_bwd (autograd of scaled_dot_product_attention, GenericTrainer.py:693-696), with the dK / dV
   partial slabs in a caller-owned buffer and their chunk-order sum on cast_stream (ordered after `stream` by an
   event): the one-pass cross-attention backward's dK / dV feed only the K / V projections' weight gradients */
int otamd_attn_bwd_ex(const AttnArgs* in, float* ws, long long ws_bytes, float* slabs, long long slab_bytes,
                      hipStream_t stream, hipStream_t cast_stream);

/* replaces: ABI check */
int otamd_attn_args_size(void);

/* replaces: the softmax inside F.scaled_dot_product_attention for heads wider than 128 (SD 1.5 160-wide heads,
   v1-inference.yaml:29-44; VAE mid-block 512-wide head): P = softmax(scale S) row-wise, bf16 P, natural-log lse */
int otamd_softmax_rows_fwd(const float* S, long long lds, void* P, long long ldp, float* lse, long long rows,
                           int ncols, int ncols_pad, float scale, hipStream_t stream);

/* replaces: autograd of that softmax: dS = scale P (dP - rowsum(P dP)) */
int otamd_softmax_rows_bwd(const void* P, long long ldp, const float* dP, long long lddp, void* dS, long long ldds,
                           long long rows, int ncols, int ncols_pad, float scale, hipStream_t stream);

/* replaces: mgds RescaleImageChannels(0..1 -> -1..1) + the NCHW image handed to AutoencoderKL.encode
   (StableDiffusionXLBaseDataLoader.py:66-67): out[b,h,w,c] = img[b,c,h,w] * mul + add, NHWC bf16, c >= C zero */
int otamd_image_to_nhwc(const float* img, int B, int C, int H, int W, float mul, float add, void* out, int cpad,
                        hipStream_t s);

/* ---- FLUX.1 transformer (rows r = t * B + b over [text ; image] tokens; modulation mod[b * ldm + off + c]) ---- */
/* replaces: AdaLayerNormZero / AdaLayerNormZeroSingle / AdaLayerNormContinuous forward (diffusers FluxTransformer2DModel,
   called at modules/modelSetup/BaseFluxSetup.py:289-299): y = LN(x) * (1 + scale[b]) + shift[b], no affine */
int otamd_adaln_fwd(const void* x, long long ldx, void* y, long long ldy, int rows, int D, float eps, const void* mod,
                    long long ldm, int shift_off, int scale_off, int B, float* mean, float* rstd, hipStream_t s);

/* replaces: autograd of that adaLN: dx, and bf16 d(shift), d(scale) written into dmod (part: otamd_mod_part_floats) */
int otamd_adaln_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long lddx, int rows,
                    int D, const void* mod, long long ldm, int shift_off, int scale_off, int B, const float* mean,
                    const float* rstd, void* dmod, float* part, hipStream_t s);

/* the same + res (the adaLN input's gradient through its residual use, the block's gated add) in the dx pass,
   instead of autograd's separate add of the two contributions */
int otamd_adaln_bwd_res(const void* x, long long ldx, const void* dy, long long lddy, const void* res, long long ldres,
                        void* dx, long long lddx, int rows, int D, const void* mod, long long ldm, int shift_off,
                        int scale_off, int B, const float* mean, const float* rstd, void* dmod, float* part,
                        hipStream_t s);

/* replaces: the modulation half of that autograd alone (bf16 d(shift), d(scale) into dmod), for a caller that runs it
   beside the dx pass on the weight-gradient stream (the modulation only feeds weight gradients) */
int otamd_adaln_dmod(const void* x, long long ldx, const void* dy, long long lddy, int rows, int D, long long ldm,
                     int shift_off, int scale_off, int B, const float* mean, const float* rstd, void* dmod, float* part,
                     hipStream_t s);

/* scratch floats the adaLN / gated-add backward reductions need */
long long otamd_mod_part_floats(int T, int D, int B);

/* replaces: hidden = hidden + gate_msa.unsqueeze(1) * attn_output (and the gate_mlp / single-block gate adds) */
int otamd_gated_add_fwd(const void* x, long long ldx, const void* y, long long ldy, void* out, long long ldo, int rows,
                        int D, const void* mod, long long ldm, int gate_off, int B, hipStream_t s);

/* replaces: autograd of the gated add: dy = gate * dout, d(gate) into dmod */
int otamd_gated_add_bwd(const void* dout, long long lddo, const void* y, long long ldy, void* dy, long long lddy,
                        int rows, int D, const void* mod, long long ldm, int gate_off, int B, void* dmod, float* part,
                        hipStream_t s);

/* replaces: ABI check */
int otamd_qk_rope_args_size(void);

/* replaces: attn.norm_q / norm_k / norm_added_q / norm_added_k (RMSNorm eps 1e-6) + apply_rotary_emb(FluxPosEmbed) */
int otamd_qknorm_rope_fwd(const QKRopeArgs* in, hipStream_t s);

/* replaces: autograd of that; optional norm-weight grads (part: >= 512 * 1024 floats) */
int otamd_qknorm_rope_bwd(const QKRopeArgs* in, void* dwq, void* dwk, void* dwq_ctx, void* dwk_ctx, int dw_f32,
                          int dw_acc, float* part, hipStream_t s);

/* replaces: GELU(approximate="tanh") of FeedForward(activation_fn="gelu-tanh") and the single blocks' act_mlp */
int otamd_gelu_tanh_fwd(const void* x, long long ldx, void* y, long long ldy, int rows, int F, hipStream_t s);

/* replaces: autograd of GELU(tanh) */
int otamd_gelu_tanh_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long lddx,
                        int rows, int F, hipStream_t s);

/* replaces: FluxModel.pack_latents (dir 0) / unpack_latents (dir 1), modules/model/FluxModel.py:317-344 */
int otamd_flux_pack(const void* src, void* dst, int B, int h, int w, int C, int ldl, int dir, hipStream_t s);

/* replaces: ResnetBlock2D norm1/norm2 + SiLU, Transformer2DModel.norm, conv_norm_out (diffusers, via BaseStableDiffusionXLSetup.py:268-273) */
int otamd_groupnorm_fwd(const void* x, long long ldx, void* y, long long ldy, int N, int HW, int C, int G,
                        float eps, const void* gamma, const void* beta, int silu, float* mean, float* rstd, float* a,
                        float* b, float* ws, hipStream_t stream);

/* replaces: autograd of GroupNorm(+SiLU) */
int otamd_groupnorm_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long lddx,
                        int N, int HW, int C, int G, const void* gamma, int silu, const float* mean, const float* rstd,
                        const float* a, const float* b, void* dgamma, void* dbeta, int param_f32, int param_acc,
                        float* ws, int accumulate, hipStream_t stream);

/* replaces: autograd of GroupNorm(+SiLU) plus the autograd add of its input's second gradient (the
   ResnetBlock2D shortcut / Transformer2DModel proj_out residual): dx = GroupNorm-backward(dy) + dres */
int otamd_groupnorm_bwd_res(const void* x, long long ldx, const void* dy, long long lddy, const void* dres,
                            long long ldres, void* dx, long long lddx, int N, int HW, int C, int G, const void* gamma,
                            int silu, const float* mean, const float* rstd, const float* a, const float* b,
                            void* dgamma, void* dbeta, int param_f32, int param_acc, float* ws, hipStream_t stream);

/* scratch floats otamd_groupnorm_fwd / _bwd need for these sizes (partial slabs, coefficients, sums) */
long long otamd_groupnorm_ws_floats(int N, int HW, int C);

/* replaces: BasicTransformerBlock norm1/norm2/norm3 */
int otamd_layernorm_fwd(const void* x, long long ldx, void* y, long long ldy, int rows, int C, float eps,
    const void* gamma, const void* beta, float* mean, float* rstd, hipStream_t stream);

/* replaces: autograd of LayerNorm */
int otamd_layernorm_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long
    lddx, int rows, int C, const void* gamma, const float* mean, const float* rstd, void* dgamma, void* dbeta,
    int param_f32, int param_acc, float* part, int accumulate, hipStream_t stream);

/* replaces: autograd of LayerNorm + the autograd add of its input's second use as the block residual
   (BasicTransformerBlock: norm1/2/3 input = to_out / ff residual): dx = LN_bwd(dy) + dres */
int otamd_layernorm_bwd_res(const void* x, long long ldx, const void* dy, long long lddy, const void* dres,
    long long ldres, void* dx, long long lddx, int rows, int C, const void* gamma, const float* mean,
    const float* rstd, hipStream_t stream);

/* replaces: the LayerNorm weight / bias gradient half of the same autograd node (dgamma = sum dy xhat,
   dbeta = sum dy), issued separately so it can run on the weight-gradient side stream */
int otamd_layernorm_param_grad(const void* x, long long ldx, const void* dy, long long lddy, int rows, int C,
    const float* mean, const float* rstd, void* dgamma, void* dbeta, int param_f32, int param_acc, float* part,
    hipStream_t stream);

/* Deferred LayerNorm parameter reduces: while a stream is in defer mode, otamd_layernorm_param_grad (and
   otamd_layernorm_bwd with parameter gradients) on it write their per-slab partials into `arena` and leave the final
   dgamma / dbeta sums pending; one grouped launch sums up to 64 of them (bit-identical to the immediate path).  The
   caller flushes before anything reads those gradients (the gradient-norm / DP bucket launches, the end of backward).
   Reference: the gamma / beta gradients of diffusers' BasicTransformerBlock norm1-3 (replaces nothing in the
   reference's own code: torch's fused LayerNorm backward reduces them inside one kernel). */
int otamd_layernorm_defer_begin(hipStream_t stream, void* arena, long long bytes);
int otamd_layernorm_defer_flush(hipStream_t stream);
int otamd_layernorm_defer_end(hipStream_t stream);
/* the same with the pending reduces launched on `launch`, which the caller has ordered after `stream` */
int otamd_layernorm_defer_end_on(hipStream_t stream, hipStream_t launch);
/* out[0] LayerNorms deferred, out[1] grouped launches (totals since load), out[2] pending on `stream` */
int otamd_layernorm_defer_stats(hipStream_t stream, long long* out);

/* replaces: diffusers GEGLU (ff.net.0) hidden * gelu(gate) */
int otamd_geglu_fwd(const void* h, long long ldh, void* out, long long ldo, int M, int F, hipStream_t s);

/* ---- text-encoder caching: CLIP-L / CLIP-bigG / T5 forward ---------------- */
/* replaces: CLIPTextEmbeddings / T5 embed_tokens (transformers, called from model/util/clip_util.py:26-31,
   t5_util.py:17-22): out[r] = tok[ids[r]] (+ pos[r % T]); ids clamped to [0, vocab) */
int otamd_embed_tokens(const long long* ids, long long n, int T, const void* tok, const void* pos, void* out, int D,
                       int vocab, hipStream_t stream);
/* replaces: CLIPMLP activation (quick_gelu CLIP-L = 0, erf gelu bigG = 1) / gelu_new (2); y may alias x */
int otamd_act_fwd(const void* x, long long ldx, void* y, long long ldy, long long rows, int C, int kind,
                  hipStream_t stream);
/* replaces: T5DenseGatedActDense's act(wi_0 x) * wi_1 x over the fused [wi_0 | wi_1] projection */
int otamd_gated_act_fwd(const void* h, long long ldh, void* out, long long ldo, long long rows, int F, int kind,
                        hipStream_t stream);
/* replaces: T5LayerNorm (RMS norm, fp32 statistics, no bias) */
int otamd_rmsnorm_fwd(const void* x, long long ldx, void* y, long long ldy, long long rows, int C, float eps,
                      const void* w, hipStream_t stream);
/* replaces: the softmax of CLIPAttention (causal mask) and T5Attention (scores + relative position bias):
   P[r] = softmax(scale S[r] + bias[q, c, h]) with r = (b H + h) Nq + q; causal masks c > q */
int otamd_softmax_masked_fwd(const float* S, long long lds, void* P, long long ldp, long long rows, int ncols,
                             int ncols_pad, float scale, int Nq, int H, int causal, const void* bias, long long bsq,
                             long long bsc, long long bsh, hipStream_t stream);

/* replaces: autograd of GEGLU */
int otamd_geglu_bwd(const void* h, long long ldh, const void* dout, long long lddo, void* dh, long long lddh,
    int M, int F, hipStream_t s);

/* replaces: nonlinearity(temb) / TimestepEmbedding act */
int otamd_silu_fwd(const void* x, void* y, long long n, hipStream_t s);

/* replaces: autograd of SiLU */
int otamd_silu_bwd(const void* x, const void* dy, void* dx, long long n, hipStream_t s);

/* replaces: torch.cat([hidden, res_hidden], dim=1) in up blocks */
int otamd_concat_channels(const void* a, long long lda, int Ca, const void* b, long long ldb, int Cb, void*
    out, long long P, hipStream_t s);

/* replaces: autograd of F.interpolate(scale_factor=2, nearest) in Upsample2D */
int otamd_upsample2x_bwd(const void* dup, void* dx, int N, int H, int W, int C, int accumulate, hipStream_t
    s);

/* replaces: bias / time_emb_proj gradients (autograd of Linear/Conv2d bias, temb broadcast add) */
int otamd_colsum(const void* x, long long ldx, int M, int N, int rows_per_group, void* out, int out_f32, int
    accumulate, float* ws, long long ws_floats, hipStream_t s);

/* replaces: workspace size query for otamd_colsum */
long long otamd_colsum_ws_floats(int M, int N, int rows_per_group);

/* replaces: weight layout transform for conv dgrad (no reference equivalent; internal) */
int otamd_conv_weight_transpose(const void* w, void* wt, int Cout, int KK, int Cin, hipStream_t s);

/* replaces: fp32 reduction result -> bf16/f32 grad (internal) */
int otamd_cast_f32(const float* x, void* y, long long n, int dst_f32, int accumulate, hipStream_t s);

/* replaces: the per-forward autocast casts of every LoRA down/up weight (LoRAModule.forward under
   autocast, modules/module/LoRAModule.py:318-322) -- one launch refreshes all bf16 shadows.
   table: device array of {long long src, dst; int rows, cols, dst_ld; float scale; int transpose, pad}
   (transpose = 1: the [rows][cols] source lands as [cols][rows] with row stride dst_ld) */
int otamd_lora_shadow(const float* src, void* dst, const void* table, int n_entries, hipStream_t s);

/* replaces: ABI check */
int otamd_lora_shadow_entry_size(void);

/* replaces: the dropout of LoRAModule.forward (modules/module/LoRAModule.py:319-323, lora_up(dropout(lora_down(x))))
   in place on t = lora_down(x) (bf16 [M, width], contiguous), and on u = dy (sB) in the backward with the same mask.
   One Philox4x32-10 call per row and group of 4 columns: Wq = ceil(width / 4), call index q = site_id * 2^40 +
   (row0 + m) * Wq + quad, counter (lo32(q), hi32(q), 6, 0x64726f70), key = *seed (device memory: a captured step
   draws a new mask on every replay); word k belongs to column 4 quad + k.  Kept iff (uint64)word >= thr, thr =
   floor(p * 2^32) in [0, 2^32]; kept -> bf16_rne(float(t) * scale), dropped -> +0.  row0 = the row of the global
   (all ranks) tensor that row 0 of t is.  site_id in [0, 2^24), (row0 + M) * Wq <= 2^40. */
int otamd_lora_dropout(void* t, long long M, int width, const unsigned long long* seed, int site_id, long long row0,
    unsigned long long thr, float scale, hipStream_t s);
/* the same mask with per-sample row numbering (the validation pass): row m of t counts as row m % rows_per of its
   sample (rows_per > 0: rows of one sample, sample-major rows) or row m / -rows_per (rows_per < 0: minus the batch
   size, token-major rows r = t * B + b), so every sample gets the mask of a batch of one on rank 0 */
int otamd_lora_dropout_per_sample(void* t, long long M, int width, const unsigned long long* seed, int site_id,
    long long rows_per, unsigned long long thr, float scale, hipStream_t s);

/* replaces: DoRAModule.forward's weight expression (modules/module/LoRAModule.py:385-412) for every adapted module in
   one launch: n = ||W + s up down|| over every axis but the kept one (axis 0: input channels, 1: output channels)
   + eps, written to `norms`, and W' = bf16(dora_scale * ((W + s up down) / n)) written to `wp` (0 where n == 0).
   Weights are [out, kk * cin] matrices in store layout; fp32 accumulation in a fixed order, no atomics.
   table: {long long w_off, wp_off, down_off, up_off, scale_off, norm_off; int out, cin, kk, rank, cblk0, rblk0;
   float s; int pad} per module, the same array on the device and on the host (the host copy is checked against the
   buffer sizes, in elements, on every call); cblk0 / rblk0: running sums of ceil(cin / 64) / ceil(out / 64).
   cin % 4 == 0, rank <= otamd_dora_max_rank(). */
int otamd_dora_merge(const void* table_dev, const void* table_host, int n, int axis, float eps, const void* base,
    long long base_numel, const float* params, long long params_numel, float* norms, long long norms_numel, void* wp,
    long long wp_numel, hipStream_t s);

/* replaces: autograd of the same expression with the norm held constant, for table entries [e0, e1): from
   g = dL/dW' (bf16, laid out as wp) to the fp32 gradients of lora_down, lora_up and dora_scale in `grads` (laid out
   as params): d_down = s up^T H, d_up = s H down^T with H = (g * dora_scale) / n, d_scale = sum g * (Weff / n);
   overwrite, or add when `accumulate` */
int otamd_dora_project(const void* table_dev, const void* table_host, int n, int e0, int e1, int axis, const void* base,
    long long base_numel, const float* params, float* grads, long long params_numel, const float* norms,
    long long norms_numel, const void* g, long long g_numel, int accumulate, hipStream_t s);

/* replaces: ABI checks */
int otamd_dora_entry_size(void);
int otamd_dora_max_rank(void);

/* replaces: the crop of mgds ScaleCropImage and RandomFlip / RandomRotate / RandomBrightness / RandomContrast /
   RandomSaturation / RandomHue between it and EncodeVAE (modules/dataLoader/mixin/DataLoaderText2ImageMixin.py:
   186-212), for every (sample, variation) of an encode batch in one call.
   table: {long long src_off, out_off; int C, Hs, Ws, y0, x0, H, W, flip; float cos_a, sin_a, brightness, contrast,
   saturation, hue} per output, the same array on the device and on the host; the host copy is checked against
   src_numel / out_numel (elements) before anything is launched.  src: flat fp32 planes [C][Hs][Ws] in [0, 1];
   out: fp32, entry i's [C][H][W] at out_off; every entry's H, W are the call's.  C = 3, or 1 (a mask: no colour
   stage).  Order: crop at (y0, x0), flip, rotate (bilinear about the crop's centre, taps outside the crop 0, positive
   angle counter-clockwise), clamp(x b), clamp(c x + (1 - c) m) with m the image's mean of 0.2989 R + 0.587 G +
   0.114 B, clamp(s x + (1 - s) gray), hue shift in turns.  A neutral stage (no rotation, 1, 1, 1, 0) is not run: a
   crop / flip entry is a bit-exact copy.  The mean is summed in a fixed order without atomics (ws: _ws_floats(n, H,
   W) floats of partial sums); two runs give the same bits.  src and out 16-byte aligned, n <= 65535. */
int otamd_image_augment(const void* table_dev, const void* table_host, int n, int H, int W, const float* src,
    long long src_numel, float* out, long long out_numel, float* ws, long long ws_floats, hipStream_t s);
long long otamd_image_augment_ws_floats(int n, int H, int W);
int otamd_aug_entry_size(void);

/* replaces: diffusers get_timestep_embedding (UNet time_proj / add_time_proj) */
int otamd_timestep_embedding(const float* t, int n, int dim, void* out, long long ldo, hipStream_t s);

/* replaces: residual add where not fused into a GEMM epilogue */
int otamd_add(const void* a, const void* b, void* y, long long n, hipStream_t s);

/* replaces: nothing (engine control): deferred split-K reduces.  Between begin and end, the split-K GEMMs launched on
   `stream` without bias / row-vector / residual operands whose output (and fused column sums) lie inside
   [out, out + out_bytes) -- the flat weight-gradient buffer, which only GEMMs on this stream write and nothing reads
   before a flush -- put their fp32 slabs into `arena` (caller-owned, 256-byte aligned, >= 1 MiB, alive until end)
   and their reduces are launched together, up to 40 per grouped launch, at flush / end, when the arena or the batch
   is full, or before a GEMM on the stream reads or writes a pending output.  Each output is summed in split order
   as by the immediate reduce: bit-identical. */
int otamd_gemm_defer_begin(hipStream_t stream, void* arena, long long bytes, const void* out, long long out_bytes);
int otamd_gemm_defer_flush(hipStream_t stream);
int otamd_gemm_defer_end(hipStream_t stream);
int otamd_gemm_defer_pending(hipStream_t stream);
int otamd_gemm_defer_stats(long long* out);

/* replaces: nothing in the reference (it has no DP): the on-chip footprint of one gradient bucket's RCCL ring
   all-reduce, emulated on one GPU for the step-slowdown measurement of DESIGN.md §6 (trainer/ddp.py
   OTAMD_DP_EMULATE): `blocks` workgroups copy `bytes` from src to dst (each wrapping over its size), paced to take
   at least `ns` nanoseconds */
int otamd_dp_emulate(const void* src, long long src_bytes, void* dst, long long dst_bytes, long long bytes, int blocks,
                     long long ns, hipStream_t s);

/* replaces: ModelSetupNoiseMixin._create_noise (modules/modelSetup/mixin/ModelSetupNoiseMixin.py:18-49) */
int otamd_noise(void* out, int f32, long long n, long long offset, unsigned long long seed, hipStream_t s);
/* replaces: the same with offset_noise_weight / perturbation_noise_weight > 0 (ModelSetupNoiseMixin.py:31-46):
   noise + ow * N[sample, channel] (constant over the pixels), then + pw * N, each op rounded to the output
   dtype in the reference's order.  NHWC tensor, hwc = h * w * C; offset = global element index of out[0]. */
int otamd_noise_ex(void* out, int f32, long long n, long long offset, unsigned long long seed, int C,
    long long hwc, float offset_weight, float perturbation_weight, hipStream_t s);
/* the deterministic noise of the validation pass: out = a whole number of NHWC samples of hwc elements, each the
   noise (offset / perturbation terms included) of a batch of one at offset 0, so a sample's noise does not depend
   on the batch or rank it is drawn in (the reference validates at batch size 1 with seed 0,
   modules/trainer/GenericTrainer.py:319-389) */
int otamd_noise_per_sample(void* out, int f32, long long n, unsigned long long seed, int C, long long hwc,
    float offset_weight, float perturbation_weight, hipStream_t s);
/* test hook: raw standard-normal draws of Philox stream `stream_id` (1 = noise, 4 = offset, 5 = perturbation) */
int otamd_noise_stream(void* out, int f32, long long n, long long offset, unsigned long long seed, int stream_id,
    hipStream_t s);

/* replaces: ModelSetupNoiseMixin._get_timestep_discrete (ModelSetupNoiseMixin.py:51-155), UNIFORM (dist 0) and
   LOGIT_NORMAL (dist 1) with static shift.  min_t / max_t = int(num_train_timesteps * min/max_noising_strength)
   (:69-70).  draws (nullable): injected per-sample draws instead of Philox -- the U[0,1) sample (UNIFORM) or the
   N(bias, weight+1) sample (LOGIT_NORMAL) of the reference's generator. */
int otamd_timesteps(int* out, int n, long long sample0, unsigned long long seed, int dist, int
    num_train_timesteps, int min_t, int max_t, float shift, float bias, float weight, const float* draws,
    hipStream_t s);
/* the same with HEAVY_TAIL (dist 2, :107-118; weight = noising_weight) and the table samplers COS_MAP / SIGMOID
   (dist 3, :119-153); dist 0 / 1 are passed on to otamd_timesteps.  All draw from the uniform of dist 0 (same Philox
   stream and counter sample0 + i, or draws[i]).  dist 3: cdf = device fp32 [n_cdf], n_cdf = max_t - min_t > 0,
   non-decreasing, last entry exactly 1.0 (util/timestep_table.timestep_cdf); out = min_t + the first index with
   cdf[index] > u (strict: a zero-weight bucket is never returned); no shift after the draw.  cdf is not read for
   dist 2. */
int otamd_timesteps_ex(int* out, int n, long long sample0, unsigned long long seed, int dist, int
    num_train_timesteps, int min_t, int max_t, float shift, float bias, float weight, const float* draws,
    const float* cdf, int n_cdf, hipStream_t s);

/* replaces: BaseStableDiffusionXLSetup.predict scale + _add_noise_discrete + get_velocity (BaseStableDiffusionXLSetup.py:214-236,277-291; ModelSetupDiffusionMixin.py:15-38) */
int otamd_ddpm_prologue(const void* latent, const void* noise, int lat_f32, const int* timestep, const float*
    acp, const float* sqrt_acp, const float* sqrt_1m, float sf, int B, long long HW, int C, int cpad, void*
    unet_in, void* target, int target_kind, float* scaled_out, hipStream_t s);

/* replaces: the same for the mask-input (inpainting) model types, with the 9-channel UNet input of
   BaseStableDiffusionXLSetup.py:217-263 / BaseStableDiffusionSetup.py:166-190 and mgds RandomLatentMaskRemove
   (DataLoaderText2ImageMixin.py:270-276), one launch.  Beside otamd_ddpm_prologue's arguments (C = 4, cpad = 16,
   target_kind 0 / 1): latent_mask f32 [B, HW], cond (the conditioning latent, unscaled) NHWC [B, HW, 4] of the
   latent's dtype, blank f32 [HW, 4] (the latent of a fully masked image of this size), unmask int32 [B].
   unet_in bf16 [B, HW, 16], 16-byte aligned: 0..3 as otamd_ddpm_prologue, 4 the mask (1 where unmask[b] != 0),
   5..8 bf16(float(cond) * sf) (bf16(blank * sf) where unmask[b] != 0), 9..15 zero.  mask_out (nullable) f32 [B, HW]:
   the mask as written to channel 4, unrounded (the loss mask of masked training). */
int otamd_inpaint_prologue(const void* latent, const void* noise, int lat_f32, const int* timestep, const float*
    acp, const float* sqrt_acp, const float* sqrt_1m, float sf, int B, long long HW, int C, int cpad, const float*
    latent_mask, const void* cond, const float* blank, const int* unmask, void* unet_in, void* target,
    int target_kind, float* scaled_out, float* mask_out, hipStream_t s);
/* the draw of mgds RandomLatentMaskRemove: out[i] = u < probability for sample sample0 + i of the global batch
   (Philox stream 8, counter = the sample's index, u in (0, 1) held below 1) */
int otamd_inpaint_unmask(int* out, int n, long long sample0, unsigned long long seed, float probability,
    hipStream_t s);
/* replaces: mgds GenerateMaskedConditioningImage (DataLoaderText2ImageMixin.py:237), on the VAE encoder's own input:
   out = bf16(float(x) * (1 - mask)), x / out NHWC bf16 [npix, cpad] in [-1, 1] (cpad % 8 == 0, 16-byte aligned),
   mask f32 [npix] in [0, 1] */
int otamd_masked_conditioning(const void* x, const float* mask, long long npix, int cpad, void* out, hipStream_t s);

/* replaces: BaseFluxSetup.predict scale/shift + ModelSetupFlowMatchingMixin._add_noise_discrete (ModelSetupFlowMatchingMixin.py:14-39) + flow target (BaseFluxSetup.py:307) */
int otamd_flow_prologue(const void* latent, const void* noise, int lat_f32, const int* timestep, float sf,
    float shift_factor, int num_t, int B, long long HW, int C, int cpad, void* model_in, void* target,
    hipStream_t s);

/* replaces: ModelSetupDiffusionLossMixin._diffusion_losses / _flow_matching_losses / __unmasked_losses + .mean()
   (ModelSetupDiffusionLossMixin.py:119-168,233-321; BaseStableDiffusionXLSetup.py:360-373; BaseFluxSetup.py:377-390).
   loss_fn: 0 CONSTANT, 1 MIN_SNR_GAMMA, 2 DEBIASED_ESTIMATION, 3 P2 (sqrt_acp / sqrt_1m tables), 4 SIGMA
   ((t+1)/num_t, flow matching).  B <= 1024. */
int otamd_mse_loss(const void* pred, int cpad, const void* target, int tgt_f32, int B, long long HW, int C,
    float mse_strength, float scale, const float* loss_weight, const int* timestep, const float* sqrt_acp,
    const float* sqrt_1m, int loss_fn, float gamma, int v_pred, int num_t, float ga, float* ws, long long ws_floats,
    float* loss_out, float* coef, float* losses_out, hipStream_t s);

/* replaces: autograd of the MSE loss */
int otamd_mse_grad(const void* pred, int cpad, const void* target, int tgt_f32, int B, long long HW, int C,
    const float* coef, const float* grad_out, void* dpred, hipStream_t s);

/* replaces: ModelSetupDiffusionLossMixin.__masked_losses / __unmasked_losses with the MSE, MAE and log-cosh terms
   (ModelSetupDiffusionLossMixin.py:27-150) + masked_losses_with_prior with masked_prior_preservation_weight == 0
   (modules/util/loss/masked_loss.py:21-37) + the scalers, loss_weight, timestep weight and .mean() of otamd_mse_loss.
   mask: float [B, HW] (one value per latent pixel, clamped to [unmasked_weight, 1], broadcast over the channels) or
   NULL (unmasked; normalize is then ignored).  A strength of exactly 0 skips its term; all three 0 is EINVAL.
   ws: float[4 * B * ceil(HW * C / 2048)].  Out: loss[1], coef[B, 3] (mse, mae, log-cosh), losses[B] (nullable). */
int otamd_diffusion_loss(const void* pred, int cpad, const void* target, int tgt_f32, const float* mask, int B,
    long long HW, int C, float mse_strength, float mae_strength, float log_cosh_strength, float unmasked_weight,
    int normalize, float scale, const float* loss_weight, const int* timestep, const float* sqrt_acp,
    const float* sqrt_1m, int loss_fn, float gamma, int v_pred, int num_t, float ga, float* ws, long long ws_floats,
    float* loss_out, float* coef, float* losses_out, hipStream_t s);

/* replaces: the host side of the reference's validation loop (modules/trainer/GenericTrainer.py:319-389:
   loss.item() per image, then a per-concept mean): adds the per-sample losses (losses_out above) of one batch and
   a count of 1 each into acc[concept_index[b]] = (sum, count), double [n_concepts][2] on the device.  One
   workgroup, no atomics, samples in ascending b, in double: equal to a sequential float64 sum on the host.
   concept_index_host (nullable): the same indices in host memory; one outside [0, n_concepts) is EINVAL before
   launch.  The kernel skips such a sample either way.  B <= 1024. */
int otamd_validation_accumulate(const float* losses, const int* concept_index, const int* concept_index_host, int B,
    int n_concepts, double* acc, hipStream_t s);

/* replaces: autograd of the loss above: dpred = m (2 d coef[b,0] + sign(d) coef[b,1] + tanh(d) coef[b,2]) grad_out[0],
   bf16, pad channels 0 */
int otamd_diffusion_loss_grad(const void* pred, int cpad, const void* target, int tgt_f32, const float* mask, int B,
    long long HW, int C, float unmasked_weight, const float* coef, const float* grad_out, void* dpred, hipStream_t s);

/* replaces: the per-step math of the sampler loop (modules/modelSampler/StableDiffusionXLSampler.py:156-172) with the
   DDIMScheduler of modules/util/create.py:1255-1266 at eta = 0, clip_sample False: p = neg + cfg (pos - neg); when
   cfg_rescale > 0, p *= 1 + cfg_rescale (std(pos) / std(p) - 1) with torch's unbiased std over the sample's 4 HW real
   elements (factor 1 for a sample whose p is constant, std(p) == 0); epsilon: x0 = (x - s1_t p) / sa_t, e = p; v_prediction: x0 = sa_t x - s1_t p, e = sa_t p + s1_t x;
   x_prev = sa_p x0 + s1_p e, with sa = sqrt_acp[.] and s1 = sqrt_1m[.] at t and t_prev (the device tables of
   NoiseScheduler.coeffs, n_table entries each).
   pred: bf16 NHWC [2B, HW, 8] = [negative | positive], 4 real channels (the pad channels are not read into anything);
   x: fp32 [B, HW, 4]; x_out: fp32 [B, HW, 4], may be x; next_in: bf16 [2B, HW, 8], both halves x_prev, pad channels 0.
   ws: otamd_cfg_ddim_step_ws_bytes(B, HW) bytes, 8-byte aligned, read only when cfg_rescale > 0.  All tensors 16-byte
   aligned.  Fixed-order reductions, no atomics: the same inputs give the same bits. */
int otamd_cfg_ddim_step(const void* pred, const float* x, float* x_out, void* next_in, int B, long long HW,
    float cfg_scale, float cfg_rescale, int v_pred, const float* sqrt_acp, const float* sqrt_1m, int n_table, int t,
    int t_prev, void* ws, long long ws_bytes, hipStream_t s);
long long otamd_cfg_ddim_step_ws_bytes(int B, long long HW);

/* replaces: VaeImageProcessor.postprocess (denormalize + numpy_to_pil's (x * 255).round()) on the decoder output
   (StableDiffusionXLSampler.py:188-189); the inverse of otamd_image_to_nhwc: x bf16 [npix, cpad] (R, G, B first) ->
   out uint8 [npix, 3] = round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even.  out 4-byte aligned. */
int otamd_nhwc_to_rgb8(const void* x, int cpad, long long npix, void* out, hipStream_t s);

/* replaces: AdamW step_adamw_parameter + addcdiv_stochastic_ (modules/util/optimizer/adamw_extensions.py:17-150; modules/util/bf16_stochastic_rounding.py:5-61), patched at modules/util/create.py:509-534 */
int otamd_adamw_bf16(void* p, const void* g, void* m, void* v, long long n, const AdamwGroup* groups, int
    n_groups, const float* clip_coef, int stochastic_rounding, unsigned long long seed, hipStream_t stream);

/* replaces: same, restricted to elements [begin, end) of the flat buffers (multiples of 8; the groups and the
   stochastic-rounding stream keep their global element indices, so chunked launches give the bits of one
   whole-store launch).  Lets the optimizer run in parameter-range chunks on its own stream. */
int otamd_adamw_bf16_range(void* p, const void* g, void* m, void* v, long long begin, long long end, const
    AdamwGroup* groups, int n_groups, const float* clip_coef, int stochastic_rounding, unsigned long long seed,
    hipStream_t stream);

/* replaces: same, fp32 parameters (LoRA weights, TrainConfig.py:959) */
int otamd_adamw_f32(void* p, const void* g, void* m, void* v, long long n, const AdamwGroup* groups, int
    n_groups, const float* clip_coef, hipStream_t stream);

/* replaces: same, fp32 master weights of a full fine-tune (weight_dtype FLOAT_32, TrainConfig.py:782, under a bf16
   autocast, dtype_util.py:28-49): p32 / m32 / v32 fp32, g16 the bf16 gradient store, w16 the bf16 working copy the
   GEMMs read, rewritten as rne(p32) (autocast's cast); elements [begin, end), multiples of 8 */
int otamd_adamw_master_range(void* p32, const void* g16, void* m32, void* v32, void* w16, long long begin,
    long long end, const AdamwGroup* groups, int n_groups, const float* clip_coef, hipStream_t stream);

/* replaces: nn.utils.clip_grad_norm_(parameters, clip_grad_norm) (modules/trainer/GenericTrainer.py:712-713);
   grad_dtype 0 bf16, 1 fp32, 2 bf16 storage of fp32-master gradients (norms and coefficient in fp32); 
   chunk_sq: double[n_chunks] scratch (one slot per chunk, summed per tensor in chunk order: deterministic) */
int otamd_grad_clip_coef(const void* grads, int grad_dtype, const void* chunks, int n_chunks, double* chunk_sq,
    double* tensor_sq, int n_tensors, float max_norm, float* out, hipStream_t stream);

/* replaces: clip_grad_norm_ split over the backward (GenericTrainer.py:712-713): squared norms of the chunks
   [c_begin, c_end) into their slots chunk_sq[c] as soon as their gradients are final (every chunk once per step),
   then the per-tensor sums in chunk order and the coefficient (out[0] coefficient, out[1] total norm) */
int otamd_grad_sqnorm_chunks(const void* grads, int grad_dtype, const void* chunks, int c_begin, int c_end,
                             double* chunk_sq, hipStream_t stream);
int otamd_grad_clip_finalize(const void* chunks, int n_chunks, const double* chunk_sq, double* tensor_sq,
                             int n_tensors, float max_norm, int grad_dtype, float* out, hipStream_t stream);

/* replaces: the grad scaling half of clip_grad_norm_ when not fused into AdamW */
int otamd_scale_bf16_by_device_scalar(void* g, long long n, const float* coef, hipStream_t stream);

/* replaces: transformers.Adafactor + patch_adafactor (modules/util/create.py:914-936), its step
   step_adafactor_parameter (modules/util/optimizer/adafactor_extensions.py:16-95) for every tensor [t_begin, t_end)
   of the table and their slabs [s_begin, s_end): factored second moments for ndim >= 2 (the last two dimensions are
   the matrix), a full second moment otherwise, update clipping by rms(u) / clip_threshold, lr * max(eps2, rms(p))
   with scale_parameter, weight decay.  form 0: p, g bf16 (round-to-nearest, or stochastic with the AdamW dither);
   1: p, g fp32; 2: p the fp32 master, g bf16, w16 the bf16 working copy rewritten as rne(p).  state: fp32 row /
   column / full states; scratch: fp32 partial sums; slab_sq: double[2 * slabs]; scal: float[4 * tensors] (rms(p),
   rms(u)); clip_coef: the pending global-norm clip (device scalar, nullable).  Five launches, no atomics. */
int otamd_adafactor_step(void* p, const void* g, void* w16, int form, float* state, float* scratch, double* slab_sq,
    float* scal, const void* tensors, int t_begin, int t_end, const void* slabs, int s_begin, int s_end,
    const AdafactorGroup* groups, int n_groups, const float* clip_coef, int stochastic_rounding,
    unsigned long long seed, hipStream_t stream);

/* replaces: ABI check */
int otamd_adafactor_tensor_size(void);
/* replaces: ABI check */
int otamd_adafactor_slab_size(void);
/* replaces: ABI check */
int otamd_adafactor_group_size(void);

/* replaces: CAME(params, lr, betas, weight_decay, eps, stochastic_rounding) (modules/util/create.py:938-951), its
   step CAME.step_parameter (modules/util/optimizer/CAME.py:79-178) for every tensor [t_begin, t_end) of the
   Adafactor tensor table, their slabs [s_begin, s_end), their fold entries [f_begin, f_end) (kinds 0, 1) and their
   row-mean entries [r_begin, r_end) (kind 2) of the fold table: factored second moments with a constant beta2,
   update clipping by rms(u) / clip_threshold, the fp32 first moment m (indexed as the store), the factored
   instability (u - m)^2 + eps2 with beta3 scaling m into the update, weight decay.  form 0: p, g bf16
   (round-to-nearest after each of the reference's two adds, or one stochastic rounding with the AdamW dither);
   1: p, g fp32; 2: p the fp32 master, g bf16, w16 the bf16 working copy rewritten as rne(p).  state_sq /
   state_res: fp32 row / column states of the second moment (and the full one of ndim < 2) and of the
   instability, indexed by the same table offsets; scratch_sq / scratch_res: their fp32 partial sums; slab_sq:
   double[slabs]; scal: float[tensors] (rms(u)); clip_coef: the pending global-norm clip (device scalar,
   nullable).  Nine launches (seven when no matrix spans slabs), no atomics. */
int otamd_came_step(void* p, const void* g, void* w16, int form, float* m, float* state_sq, float* state_res,
    float* scratch_sq, float* scratch_res, double* slab_sq, float* scal, const void* tensors, int t_begin, int t_end,
    const void* slabs, int s_begin, int s_end, const void* fold, int f_begin, int f_end, int r_begin, int r_end,
    const CameGroup* groups, int n_groups, const float* clip_coef, int stochastic_rounding, unsigned long long seed,
    hipStream_t stream);

/* replaces: ABI check */
int otamd_came_group_size(void);
/* replaces: ABI check */
int otamd_came_fold_size(void);

/* replaces: the state pass of prodigyopt.Prodigy.step as modules/util/create.py:863-881 builds it (the package is
   not in the reference tree: the contract is the published step, restated in tests/_oracle_prodigy.py).  One
   workgroup per NormChunk of the grad-norm chunk table (8-aligned begin, at most 65536 elements, inside one tensor;
   the caller checked the ranges): with g the gradient after the pending clip (clip_coef, nullable; bf16-rounded in
   form 0) plus weight_decay p in the coupled form, and d, k read from `state`: num += g (p0 - p) (fp32 difference,
   fp64 product and sum), m = beta1 m + d (1 - beta1) g (beta1 > 0; m may be null otherwise), v = beta2 v +
   d^2 (1 - beta2) g g, s = beta3 s + a g with a = (d / d0) dlr or (d / d0) d under safeguard_warmup, den += |s|;
   chunk_num[c], chunk_den[c]: one fp64 slot per chunk, no atomics.  p0 / m / v / s: fp32, indexed as the store.
   form 0: p, g bf16; 1: p, g fp32; 2: p the fp32 master, g bf16.  capture_p0: the first step, p0 = p is written
   instead of read.  One launch. */
int otamd_prodigy_accumulate(const void* p, const void* g, int form, float* p0, float* m, float* v, float* s,
    const void* chunks, int n_chunks, double* chunk_num, double* chunk_den, const void* state,
    const ProdigyHyper* hyper, const float* clip_coef, int capture_p0, hipStream_t stream);

/* replaces: the scalar part of Prodigy.step: one workgroup folds the chunk slots in a fixed order and updates
   `state` (device ProdigyState) in fp64: d_numerator = beta3 d_numerator + (d / d0) dlr num, d_denom = den; den == 0
   sets skip and changes nothing else; otherwise d_hat = d_coef d_numerator / d_denom, d = max(d, d_hat) while
   d == d0, d_max = max(d_max, d_hat), d = min(d_max, d growth_rate), k += 1, skip = 0.  One launch. */
int otamd_prodigy_finalize(const double* chunk_num, const double* chunk_den, int n_chunks, void* state,
    const ProdigyHyper* hyper, hipStream_t stream);

/* replaces: the parameter update of Prodigy.step over the n elements of the store (a multiple of 8), reading d, dlr
   and skip from `state`: nothing when skip; else p += (-weight_decay dlr) p (decoupled form), p -= dlr m /
   (sqrt(v) + d eps) with the new d and the step's dlr; beta1 == 0: d g stands for m (g, clip_coef as accumulate saw
   them).  form as above; w16: the bf16 working copy of form 2, rewritten as rne(p); form 0 rounds to nearest or
   stochastically (the AdamW dither on the element index).  Workgroup cap OTAMD_ADAMW_BLOCKS.  One launch. */
int otamd_prodigy_apply(void* p, void* w16, const void* g, int form, const float* m, const float* v, long long n,
    const void* state, const ProdigyHyper* hyper, const float* clip_coef, int stochastic_rounding,
    unsigned long long seed, hipStream_t stream);

/* replaces: ABI check */
int otamd_prodigy_state_size(void);
/* replaces: ABI check */
int otamd_prodigy_hyper_size(void);

/* replaces: the non-foreach path of schedulefree.AdamWScheduleFree.step as modules/util/create.py:752-767 builds it
   (the package is not in the reference tree: the contract is the step restated in tests/_oracle_schedule_free.py).
   Over elements [begin, end) (multiples of 8) of a store of n elements, per group (at most 8, sorted, disjoint), with
   g the gradient after the pending clip (clip_coef, nullable; bf16-rounded in form 0): v = beta2 v + (1 - beta2) g g,
   gn = g / (sqrt(v inv_bc2) + eps) + weight_decay y, y = y + ckp1 (z - y), y = y + a_y gn, z = z - lr gn; every fp32
   operation one rounding, no fused multiply-add.  z / v: fp32, indexed as the store; elements outside every group
   (the store's padding) are not written.  form 0: p, g bf16, rounded to nearest or stochastically (the AdamW dither
   on the element index); 1: p, g fp32; 2: p the fp32 master, g bf16, w16 the bf16 working copy rewritten as rne(p).
   Workgroup cap OTAMD_ADAMW_BLOCKS.  One launch, no atomics. */
int otamd_sf_adamw_step(void* p, void* w16, const void* g, int form, float* z, float* v, long long n, long long begin,
    long long end, const SfGroup* groups, int n_groups, const float* clip_coef, int stochastic_rounding,
    unsigned long long seed, hipStream_t stream);

/* replaces: AdamWScheduleFree.eval() / .train() (p.lerp_(z, 1 - 1/beta1) / p.lerp_(z, 1 - beta1)), called by
   modules/trainer/GenericTrainer.py:414-449, 470-483, 772-775 around every backup and save: p = p + w (z - p) over
   the groups' ranges inside [begin, end).  Forms as above; form 0 always rounds to nearest (a mode switch is
   repeatable).  One launch. */
int otamd_sf_swap(void* p, void* w16, int form, const float* z, long long n, long long begin, long long end,
    const SfSwapGroup* groups, int n_groups, hipStream_t stream);

/* replaces: ABI check */
int otamd_sf_group_size(void);
/* replaces: ABI check */
int otamd_sf_swap_group_size(void);

/* replaces: bnb.optim.AdamW8bit.step as modules/util/create.py:553-566 builds it (block-wise, two states, blocks of
   256, dynamic-tree codebooks; bitsandbytes is not in the reference tree: the contract is the step restated in
   tests/_oracle_adamw8bit.py).  One launch over every tensor of the table, one wave per block: m = map1[code1] absmax1,
   v = map2[code2] absmax2 (tensors with is8bit 0 read fp32 m, v from m32 / v32), m = beta1 m + (1 - beta1) g,
   v = beta2 v + ((1 - beta2) g) g, p = (p + step_size (m / (sqrt(v) + eps_c))) wd_factor, new absmax = max |m|, max v
   over the block, new codes = the number of codebook midpoints strictly below m / absmax (0 / 0 taken as 0); every
   fp32 operation one rounding, no fused multiply-add.  g after the pending clip (clip_coef, nullable; bf16-rounded in
   form 0).  code1 / code2: uint8 indexed as the store (n elements; the padding is never written); absmax1 / absmax2:
   n_absmax fp32; m32 / v32: n_f32 fp32; qmap: 512 fp32 on the device, the signed then the unsigned codebook, each
   ascending.  table_dev / table_host: the same A8Seg[n_segs] on the device and on the host; the host copy is checked
   on every call (otamd_adamw8bit_check) before anything is launched.  Forms as otamd_sf_adamw_step.  Workgroup cap
   OTAMD_ADAMW_BLOCKS.  No atomics. */
int otamd_adamw8bit_step(void* p, void* w16, const void* g, int form, void* code1, void* code2, float* absmax1,
    float* absmax2, long long n_absmax, float* m32, float* v32, long long n_f32, const float* qmap, long long n,
    const void* table_dev, const void* table_host, int n_segs, const A8Group* groups, int n_groups,
    const float* clip_coef, int stochastic_rounding, unsigned long long seed, hipStream_t stream);

/* replaces: nothing (the table check of otamd_adamw8bit_step, host code only: tensors sorted, disjoint and inside
   the store of n elements, work blocks numbered consecutively from 0, state ranges of one kind ascending, disjoint and
   inside their buffers, group < n_groups; OTAMD_EINVAL otherwise) */
int otamd_adamw8bit_check(const A8Seg* table, int n_segs, long long n, long long n_absmax, long long n_f32,
    int n_groups);

/* replaces: ABI check */
int otamd_adamw8bit_seg_size(void);
/* replaces: ABI check */
int otamd_adamw8bit_group_size(void);

/* replaces: EMAModuleWrapper.step (modules/module/EMAModule.py:37-54), ema.add_(one_minus_decay * (parameter - ema))
   per tensor, for elements [begin, end) of the flat buffers (multiples of 8, 16-byte aligned pointers; padding is 0
   in both and stays 0).  Each of the three torch ops rounds to its result dtype.  form 0: ema, p bf16; 1: ema, p
   fp32 (an fp32 store or the master of a master store); 2: ema fp32, p bf16 widened exactly (torch's promotion
   after ema.to(dtype=float32)).  one_minus_decay: Python's double 1 - decay narrowed to fp32.  One launch. */
int otamd_ema_range(void* ema, const void* p, int form, long long begin, long long end, float one_minus_decay,
    hipStream_t stream);

/* replaces: nothing (the elements one sweep of the grid-stride loop of form's EMA kernel covers at the grid cap) */
int otamd_ema_sweep_elems(int form);

#ifdef __cplusplus
}
#endif
#endif /* OTAMD_H */
