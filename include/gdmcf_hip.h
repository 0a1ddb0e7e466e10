/* gdmcf_hip.h -- C ABI of libgdmcf_hip.so, the MI355X (gfx950) hot path of GDMCF.
 *
 * The reference (GDMCF/GDMCF, pure Python on PyTorch) has NO FFI / plugin interface
 * (SURVEY.md F1): its boundary is the Python object protocol between main.py and the classes
 * GaussianDiffusion / DNN / LightGCN.  This header is the C boundary a maintainer would bind
 * underneath those classes; every entry point names the reference code it replaces
 * (file:line relative to the reference root).  gdmcf_amd/ (Python, ctypes) is that binding.
 *
 * Conventions
 *   - plain pointers + sizes; all `const float*`/`float*`/`int64_t*` arguments are DEVICE
 *     pointers unless the name ends in `_host`; no torch types.
 *   - matrices are row-major; `ld*` is the row stride in ELEMENTS (may exceed the width).
 *   - every device function enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns immediately: 0 = ok, negative = error (GDMCF_E_*); the Python layer maps
 *     GDMCF_E_SHAPE to AssertionError, GDMCF_E_ARG to ValueError, GDMCF_E_UNSUPPORTED to
 *     NotImplementedError (the reference's own error conventions) and
 *     GDMCF_E_HIP to RuntimeError.
 *   - no function allocates device memory; scratch is passed in as `ws`/`ws_bytes`
 *     (query the size with the matching *_ws_bytes function) so everything is
 *     hipGraph-capturable.
 *   - random draws: every in-kernel draw is a function of words of ONE Philox4x32-10 block, named below by its counter
 *     (position, row, stream, offset) and the key `seed` (low word, high word).  The four counter words are
 *         (position, row, stream | (offset >> 32) << 8, offset & 0xFFFFFFFF):
 *     stream ids are below 256 and a Philox `offset` is below 2^56 (GDMCF_E_SHAPE otherwise, from every entry that takes
 *     one) -- its bits 32..55 sit above the stream id, so offsets that differ only in their high bits draw different
 *     numbers, and an offset below 2^32 gives the counter (position, row, stream, offset) itself.  Checkpoints persist
 *     (seed, offset): the mapping is a stored format.
 */
#ifndef GDMCF_HIP_H
#define GDMCF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDMCF_OK 0
#define GDMCF_E_SHAPE (-1)       /* shape/assert violation  -> AssertionError      */
#define GDMCF_E_ARG (-2)         /* bad enum / value        -> ValueError          */
#define GDMCF_E_UNSUPPORTED (-3) /* unknown schedule etc.   -> NotImplementedError */
#define GDMCF_E_HIP (-4)         /* HIP runtime error       -> RuntimeError        */
#define GDMCF_E_WORKSPACE (-5)   /* workspace too small     -> RuntimeError        */

/* library / device ------------------------------------------------------------------ */
int gdmcf_version(void);                 /* ABI version, currently 1 */
const char* gdmcf_last_error(void);      /* thread-local message of the last failing call */
int gdmcf_device_info(int* n_cu, int* wave_size, char* arch_host, int arch_len);
/* Which kernel family the calling thread's LAST dense product was dispatched to (introspection for tests and
 * profiles -- "did the hand-written path run?"): 1 LDS-tiled f32 MFMA kernel, 2 register-streaming weight-gradient
 * kernel, 3 the same with the AdamW stream, 4 fat-tile output-layer kernel (one tile per wave), 5 register-streaming
 * input-gradient / cached-W^T forward kernel (dr_kn_kernel), 6 fat-tile kernel over split-K slabs (the first-layer forward), 7 bf16-input kernels,
 * 8 f32x3 kernels, 9 element-wise kernel for degenerate shapes; 0 none yet.                              */
int gdmcf_debug_last_gemm(void);
/* What the fat-tile slab route (family 6) plans for gdmcf_linear_fwd_f32's product C[M, N] = A[M, K] W[N, K]^T on the current device, in
 * the calling thread's GEMM precision: returns 1 and the tile width *nb (x 16 columns), the split count *splits and the chunks of
 * 16 k per split *cps, or 0 (all three 0) when the route does not take the shape.  The call itself may still decline: a workspace
 * that is not 16-byte aligned or smaller than gdmcf_linear_ws_bytes.  Tests pick their shapes with it. */
int gdmcf_debug_fat_slab_plan(int M, int N, int K, int* nb, int* splits, int* cps);
/* What the register-streaming weight-gradient kernels (families 2 and 3) plan for dW[N, K] = dZ[M, N]^T A[M, K] in float32 mode,
 * host only, nothing launched.  bias_col != 0: the call asks for db as column K of the product (a_scale_col != 0 with db given; it
 * needs lda > K); fused != 0: the plan of gdmcf_linear_bwd_weight_adamw_f32, else of gdmcf_linear_bwd_weight_f32.  Returns 1 and the
 * ring depth *depth (7, 8 or 9), the k-steps of 4 batch rows a tile runs *ksp (a multiple of depth + 1; ksp - ceil(M / 4) of
 * them are padded steps that read past the operands), the 64 x 64 tiles along N and along K (the bias column counted) *tiles_m and
 * *tiles_n, the ticket order *m_fastest and whether the product carries the bias column *has_bias -- or 0 (all six 0) when the
 * kernels do not take the shape or their route is switched off.  A fused product updates W inside the k loop of the next tile when
 * ksp / (depth + 1) >= 9, else at the end of its own tile. */
int gdmcf_debug_dr_tn_plan(int M, int N, int K, int64_t lddz, int64_t lda, int64_t ldw, int bias_col, int fused, int* depth,
                           int* ksp, int* tiles_m, int* tiles_n, int* m_fastest, int* has_bias);

/* Optional in-library timing with HIP events on the launch stream (bench.py's live roofline
 * measurement).  While enabled, every tagged kernel launch is bracketed by two hipEventRecord
 * calls; gdmcf_prof_collect synchronises them and returns (tag, milliseconds, work) triples,
 * where work = algorithmic FLOPs (GEMM tags) or bytes (HBM-bound tags) of that launch.
 * Tags: 1 linear_fwd gemm, 2 loss_fwd gemm, 3 posterior gemm, 4 bwd_input gemm, 5 bwd_weight gemm,
 * 6 adamw (also normalize_rows_bwd_adamw / scatter_rows_adamw), 7 prep_input, 8 spmm, 9 topk, 12 score_topk and score_rank (work = the
 * 2 n_rows n_items d FLOPs of the score product, per pass).
 * on: 1 = record, 2 = pause (stop recording, keep the records), 0 = off and discard.           */
int gdmcf_prof_enable(int on);
int gdmcf_prof_collect(int cap, int* tags_host, float* ms_host, double* work_host);

/* ---- schedules: host, float64 --------------------------------------------------------
 * replaces GaussianDiffusion.get_betas + calculate_for_diffusion
 * (models/gaussian_diffusion.py:109-159, betas_from_linear_variance :1138-1144,
 * betas_for_alpha_bar :1146-1163, betas[0]=1e-5 :79).
 * kind: 0 linear, 1 linear-var, 2 cosine, 3 binomial.
 * out_tables_host: [13][T] doubles in this order: betas, alphas_cumprod, alphas_cumprod_prev,
 * alphas_cumprod_next, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod,
 * log_one_minus_alphas_cumprod, sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 * posterior_variance, posterior_log_variance_clipped, posterior_mean_coef1, posterior_mean_coef2.
 * Returns GDMCF_E_SHAPE when the reference's asserts (:81-83) would fire. */
#define GDMCF_N_TABLES 13
int gdmcf_schedule_build(int kind, double noise_scale, double noise_min, double noise_max, int T,
                         int beta_fixed, double* out_tables_host);

/* ---- batch provider: dense user rows from a device-resident CSR interaction matrix ----------
 * replaces DataDiffusion.__getitem__ + DataLoader collation + batch.to(device)
 * (data_utils.py:216-226, main.py:155,343): out[b, 0:I] = dense row row_ids[b] (row_ids NULL -> b).
 * indptr int64 [n_users+1], indices int32, values float32 or NULL (all ones); rows must hold each
 * column at most once (scipy's csr_matrix constructor has already summed duplicates).  Columns
 * outside [0, I) are skipped.  values and row_ids are optional; indptr, indices and out are
 * required (GDMCF_E_ARG).                                                                    */
int gdmcf_densify_rows_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                           const int64_t* row_ids, int B, int I, float* out, int64_t ldo, void* stream);

/* ---- denoiser input: q_sample + F.normalize + dropout + timestep embedding + cat ------
 * replaces GaussianDiffusion.q_sample (:399-407) with _extract_into_tensor (:532-547),
 * and DNN.forward's prologue (models/DNN.py:73-78): timestep_embedding (:1806-1825),
 * emb_layer, F.normalize, nn.Dropout, torch.cat.
 *   xin[b, 0:I]   = drop( norm( ca[ts[b]]*x[b,:] + cb[ts[b]]*noise[b,:] ) )
 *   xin[b, I:I+E] = emb_w @ temb(ts[b]) + emb_b ;  xin[b, I+E:ldxin] = 0
 * ca/cb: float32 tables [T] (the reference casts the f64 tables to f32 before use); pass
 * NULL for both to skip the q_sample (xin <- x).
 * noise_mode 0: none (requires ca==NULL or cb treated as 0); 1: explicit `noise` [B,ldn];
 *            2: Philox4x32-10 + Box-Muller N(0,1): element (b,i) is component i&3 of the block with
 *               counter (i>>2, b, stream, offset) and key seed (stream 0 = noise, 1 = dropout),
 *               so any kernel can regenerate it.
 * drop_mode  0: none; 1: explicit keep-mask `keep` (uint8 [B,ldkeep]); 2: Philox Bernoulli(1-p): element (b,i) is kept iff its
 *               16-bit uniform < round((1-p) * 65536) (the keep probability is quantised to 2^-16: exact for p = 0.5; the scale
 *               1/(1-p) is not quantised); the uniform is half (i >> 10) & 1 (low, high) of word i & 3 of the stream-1 block with
 *               counter ((i & ~1024) >> 2, b, 1, offset): one block serves the eight elements i..i+3 and i+1024..i+1027.
 * normalize != 0 applies F.normalize (L2, eps 1e-12) to the (noised) row before dropout and
 * needs rownorm_ws (float32 [B] scratch).
 * xt_out (optional, [B,ldxt]) receives the pre-normalize/pre-dropout x_t.
 * temb_out (optional, [B,E]) receives the sinusoidal embedding (needed by the backward).   */
int gdmcf_dnn_prep_input_f32(const float* x, int64_t ldx, const int64_t* ts, const float* ca,
                             const float* cb, int noise_mode, const float* noise, int64_t ldn,
                             int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p,
                             uint64_t seed, uint64_t offset, int normalize, const float* emb_w,
                             const float* emb_b, int E, int B, int I, float* xin, int64_t ldxin,
                             float* xt_out, int64_t ldxt, float* temb_out, float* rownorm_ws,
                             void* stream);
/* The same builder fed from a device-resident CSR matrix of {0,1} interactions instead of dense
 * rows: row b of the batch is row rows[b] of (indptr int64, indices int32).  Nothing dense is read: a workgroup marks its
 * 4096 columns of the row in an LDS bitmap and builds x_t = ca*x0 + cb*noise, dropout, the embedding columns from it
 * (same arithmetic and the same Philox streams as the dense entry: identical xin).  bits_out (optional, uint32
 * [B, ldbits], ldbits >= ceil(I/32)) receives the rows as bitmaps -- the target of gdmcf_linear_loss_fwd_bits_f32.
 * Indices outside [0, I) are ignored, as gdmcf_densify_rows_f32 skips them: they add nothing to xin and set no bit of
 * bits_out (every bit >= I of a written word is zero); an index stored twice counts once.
 * No F.normalize here (it needs the dense row twice): densify (gdmcf_densify_rows_f32) and use the dense entry.        */
int gdmcf_dnn_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts,
                                 const float* ca, const float* cb, int noise_mode, const float* noise, int64_t ldn,
                                 int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed,
                                 uint64_t offset, const float* emb_w, const float* emb_b, int E, int B, int I, float* xin,
                                 int64_t ldxin, float* temb_out, uint32_t* bits_out, int64_t ldbits, void* stream);

/* ---- one-hot rows with discrete transition noise (first slice) -------------------
 * replaces GaussianDiffusionDiscrete.apply_noise (gaussian_diffusion.py:770-831: get_Qt_bar :597-614,
 * sample_discrete_features :999-1038) together with F.one_hot(x_start) and the `x_tU & one_hot(x_start)` that
 * follows it (:841-849 in training_losses, :672-686 in p_sample), and the x_U.reshape of DNNOneHot.forward
 * (models/DNN.py:444):
 *   c0 = x0[b,i] != 0 ; s ~ row c0 of Q = a*I + (1-a)*[[e,1-e],[e,1-e]], a = (float)ts[b]/B (:775), e = discrete ;
 *   xU[b, 2i + c] = (c == c0 && s == c0) ? 1 : 0          (float32, the [B, 2I] input of the second MLP branch)
 * sampled (optional, uint8 [B,lds]): the drawn classes s are given (parity runs; ts may be NULL then); otherwise
 * s = (u < P(1)) with u the Philox4x32-10 uniform of element (b,i): component i&3 of the block with counter
 * (i>>2, b, 3, offset), key seed.  sampled_out (optional) receives s.                                        */
int gdmcf_onehot_noise_f32(const float* x0, int64_t ldx, const int64_t* ts, int B, int I, float discrete,
                           const uint8_t* sampled, int64_t lds, uint64_t seed, uint64_t offset,
                           float* xU, int64_t ldu, uint8_t* sampled_out, int64_t ldso, void* stream);
/* The second branch's first-layer input straight from device CSR rows: replaces, for training on rows that stay sparse,
 * the same reference lines as gdmcf_onehot_noise_f32 (gaussian_diffusion.py:841-849, :770-831, models/DNN.py:444) together
 * with the input builder of branch 2 (models/DNN.py:446-455: dropout, timestep embedding, cat) -- in ONE launch, for row b =
 * row rows[b] of the {0,1} matrix (indptr int64, indices int32):
 *   xin[b, :] = [ drop( xU[b, 0:2I] ) | emb_w @ temb(ts[b]) + emb_b (E columns) | 1 | 0 up to ldxin ]
 * with xU as defined above, i.e. exactly what gdmcf_onehot_noise_f32 followed by gdmcf_dnn_prep_input_f32(I = 2I, ca = cb = NULL,
 * normalize = 0) leave in xin -- bit for bit, for equal inputs, seed and offsets -- without xU and without any dense row.
 * Class draws: `sampled` given (ts_U may be NULL), or drawn with the counters of gdmcf_onehot_noise_f32 (stream 3) at
 * offset_noise from a = (float)ts_U[b]/B; sampled_out (optional, uint8 [B, ldso]) receives them.  Dropout over the 2I columns:
 * drop_mode / keep / drop_p as gdmcf_dnn_prep_input_f32 (stream 1) at offset_prep.  ts: the timesteps of the embedding
 * columns; temb_out as there.  bits_out (optional): the rows as bitmaps, as gdmcf_dnn_prep_input_csr_f32 writes them.
 * Both offsets are by-value: the entry refuses to run while a graph step state is bound (gdmcf_graph_state_bind).            */
int gdmcf_onehot_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts_U,
                                    float discrete, const uint8_t* sampled, int64_t lds, uint64_t seed, uint64_t offset_noise,
                                    uint8_t* sampled_out, int64_t ldso, const int64_t* ts, int drop_mode, const uint8_t* keep,
                                    int64_t ldkeep, float drop_p, uint64_t offset_prep, const float* emb_w, const float* emb_b,
                                    int E, int B, int I, float* xin, int64_t ldxin, float* temb_out, uint32_t* bits_out,
                                    int64_t ldbits, void* stream);

/* ---- N(0,1) fill --------------------------------------------------------------------------------
 * replaces `noise = th.randn_like(x_start)` where the noise itself is needed in memory: the eps TARGET of
 * training_losses (gaussian_diffusion.py:328-331, :844-846) and the reverse loop's `noise = th.randn_like(x_t)`
 * (:210-217, :696-703).  out[b, i] (float32 [rows, ld]) = normal (i & 3) of the Philox4x32-10 block with counter
 * (i >> 2, b, stream_id, offset) (all 56 offset bits count: Conventions), key seed: Box-Muller on the block's (x, y) and
 * (z, w) words, hardware log / sqrt / sin / cos.  stream_id 0 is the stream gdmcf_dnn_prep_input(_csr)_f32 draws in place (noise_mode 2): a buffer filled here
 * with the same (seed, offset) and handed to it as given noise (noise_mode 1) yields the same x_t bit for bit.  Stream ids
 * 1-3, 5, 6 belong to dropout / timestep / one-hot / graph draws; 4 and 7 are free for callers (eps target, step noise).  */
int gdmcf_randn_f32(float* out, int64_t ld, int rows, int cols, int stream_id, uint64_t seed, uint64_t offset, void* stream);

/* ---- loss target of the eps parameterisation ---------------------------------------------------
 * replaces the element-wise passes of training_losses for ModelMeanType.EPSILON (gaussian_diffusion.py:328-348):
 *   target[b,:] = noise[b,:]                      alpha[b] = 1       rowdiv[b] = I      (t != 0, or t0_likelihood == 0)
 *   target[b,:] = r1[0]*x_t[b,:] - x0[b,:]         alpha[b] = r2[0]   rowdiv[b] = 2 I    (t == 0: the x0-likelihood row, :344-348)
 * (product and difference rounded separately, as torch's mul and sub).  alpha / rowdiv feed gdmcf_linear_loss_fwd_f32 and
 * gdmcf_row_loss_finish_*.  target may equal noise (same leading dimension): only the t == 0 rows are written then.      */
int gdmcf_eps_target_f32(const float* noise, int64_t ldn, const float* xt, int64_t ldxt, const float* x0, int64_t ldx0,
                         const int64_t* ts, const float* r1, const float* r2, int t0_likelihood, int B, int I, float* target,
                         int64_t ldt, float* alpha, float* rowdiv, void* stream);

/* ---- degree-guided graph of the reverse loop (gaussian_diffusion.py:706-729, inside GaussianDiffusionDiscrete.p_sample) ----
 * One reverse step's update of the accumulated user-item graph, one byte per edge state:
 *   s[b,i] ~ row c of Q = a*I + (1-a)*[[e,1-e],[e,1-e]], c = graph[b,i], a = (float)ts[b]/B, e = discrete   (apply_noise on
 *            the accumulated one-hot graph, :709);
 *   pick[b] ~ Bernoulli(degree_prob[b]), degree_prob = row sum / largest row sum of x_start   (multinomial(1), :710-716);
 *   graph[b,i] |= s[b,i] & (user_guided ? pick[b] : 1)                                          (:719-727).
 * sampled_in / pick_in (optional, uint8): the draws are given (parity runs); otherwise Philox4x32-10, key seed, counters
 * (i>>2, b, 5, offset) for the classes and (0xFFFFFFFF, b, 6, offset) for the user bit.  sampled_out / pick_out
 * (optional) receive the draws.  The graph is what the reference hands to the denoiser as `graph=` (:744).              */
int gdmcf_graph_guided_step_u8(uint8_t* graph, int64_t ldg, const int64_t* ts, int B, int I, float discrete,
                               const uint8_t* sampled_in, int64_t lds, const uint8_t* pick_in, const float* degree_prob,
                               int user_guided, uint64_t seed, uint64_t offset, uint8_t* sampled_out, int64_t ldso,
                               uint8_t* pick_out, void* stream);

/* Rewrites only the embedding + padding columns [I, ldxin) of xin for new timesteps (reverse
 * loop: x_t already sits in xin[:, 0:I], written by gdmcf_linear_posterior_fwd_f32).          */
int gdmcf_dnn_emb_cols_f32(const int64_t* ts, const float* emb_w, const float* emb_b, int E, int B,
                           int I, float* xin, int64_t ldxin, float* temb_out, void* stream);

/* ---- dense layers on the f32 MFMA (v_mfma_f32_16x16x4_f32) -------------------------------
 * replaces nn.Linear (+tanh) in DNN.forward (models/DNN.py:79-86) and their autograd backward
 * (main.py:350).  W is nn.Linear layout [N,K].  act: 0 none, 1 tanh.                        */
/* Input precision of the dense products (BASELINE configs[2] "bf16 denoiser GEMM on MFMA").  The setting is
 * per calling thread and applies to every gdmcf_linear_* call that follows; returns the previous mode (a mode
 * outside the enum only queries).  GDMCF_GEMM_BF16: both operands of each product are rounded to bfloat16
 * (nearest-even) on chip and multiplied on the bf16 matrix pipe with float32 accumulation; all tensors in HBM
 * (weights, activations, gradients, optimiser state) stay float32.  Replaces what the reference would obtain
 * with torch.autocast(dtype=torch.bfloat16) around models/DNN.py:79-86 -- the reference itself runs fp32.
 * GDMCF_GEMM_F32X3: float32 products on the bf16 matrix pipe -- every operand is split on chip into three bfloat16
 * terms (a = a0 + a1 + a2, exact to 2^-26 |a|) and each product is assembled from the six partial products above
 * 2^-25 |a b| with float32 accumulation: float32-level error (no operand is rounded), 2.67x the matrix-pipe rate of
 * v_mfma_f32_16x16x4_f32; non-finite inputs give NaN.  No shadows, nothing extra in HBM.                     */
enum { GDMCF_GEMM_F32 = 0, GDMCF_GEMM_BF16 = 1, GDMCF_GEMM_F32X3 = 2 };
int gdmcf_gemm_precision(int mode);
/* bf16 shadows (GDMCF_GEMM_BF16 only): a shadow is a bfloat16 copy of a float32 matrix that the library may
 * stream INSTEAD of the float32 matrix when that matrix is an operand of a dense product (half the bytes, no
 * conversion on chip), and that these library kernels keep up to date when they write the float32 matrix:
 * gdmcf_dnn_prep_input_f32 / gdmcf_dnn_emb_cols_f32 (xin), gdmcf_linear_fwd_f32 (C), gdmcf_linear_loss_fwd_f32
 * (diff), gdmcf_linear_posterior_fwd_f32 (x_next), gdmcf_linear_bwd_input_f32 (dA), gdmcf_rowscale_f32 (out),
 * gdmcf_adamw_bf16s_f32 and gdmcf_linear_bwd_weight_adamw_f32 (W).  The float32 matrix stays authoritative; a
 * shadow whose float32 matrix was written by anything else must be refreshed with gdmcf_bf16_shadow_sync.  Layout: [round_up(rows, 64)][ld_bf16] bfloat16, ld_bf16 a multiple of 64
 * and >= cols, 16-byte aligned, ZERO outside [rows, cols) (the kernels rely on the zero padding instead of edge
 * predicates).  The registry is keyed by the float32 base pointer and global to the process: clear an entry
 * before its buffers are freed.  A product uses shadows only when BOTH operands have one of exactly its shape. */
int gdmcf_bf16_shadow_set(const float* f32, void* bf16, int64_t rows, int64_t cols, int64_t ld_bf16);
int gdmcf_bf16_shadow_clear(const float* f32 /* NULL: all */);
void* gdmcf_bf16_shadow_get(const float* f32);
/* 1 and the registered description, or 0 when `f32` has no shadow */
int gdmcf_bf16_shadow_info(const float* f32, void** bf16, int64_t* rows, int64_t* cols, int64_t* ld_bf16);
int gdmcf_bf16_shadow_sync(const float* f32, int64_t ld, void* stream);
size_t gdmcf_linear_ws_bytes(int M, int N, int K);
/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias) */
int gdmcf_linear_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw,
                         const float* bias, int act, int M, int N, int K, float* C, int64_t ldc,
                         void* ws, size_t ws_bytes, void* stream);
/* The same layer with the weight given TRANSPOSED: Wt[K, N] row-major (ldwt >= N), out = act(A @ Wt + bias).  For loops over
 * FROZEN weights (the reverse-diffusion loop of evaluation, gaussian_diffusion.py:161-220 over models/DNN.py:79-81): with a
 * K-contiguous A and an N-contiguous Wt the product runs on the register-streaming kernel of the input gradient (both operands
 * straight into the MFMA layout, no LDS).  The caller keeps Wt equal to W^T; float32 GEMM mode only; ws as gdmcf_linear_ws_bytes. */
int gdmcf_linear_fwd_wt_f32(const float* A, int64_t lda, const float* Wt, int64_t ldwt,
                            const float* bias, int act, int M, int N, int K, float* C, int64_t ldc,
                            void* ws, size_t ws_bytes, void* stream);
/* A first hidden layer on a sparse {0,1} input row, as a sum of table rows: replaces the first nn.Linear (+tanh) of
 * DNN.forward (models/DNN.py:79-81) and of both branches of DNNOneHot.forward (:446-455) where the layer's input is known to
 * be binary and undropped -- the first reverse step of an evaluation with sampling_steps == 0 (x_T is x_0 itself), and the
 * one-hot backbones' second branch at every reverse step (its image is the noiseless one-hot of x_0 for the whole loop):
 *   out[b, n] = act( pre[b, n] + base[n] + sum_{j in CSR row rows[b]} table[j, n] + sum_{e < E} a[b, e] * tblE[e, n] + bias[n] )
 * Every operand is optional (NULL), but one of pre / the CSR rows / a must be given.  pre [B, ldpre]; base, bias [N]; the CSR
 * rows are rows[b] of (indptr int64, indices int32) as in gdmcf_dnn_prep_input_csr_f32, indptr == NULL: no gather; table
 * [I, ldt] and tblE [E, ldte] are row-major with N-contiguous rows (W^T, the orientation gdmcf_linear_fwd_wt_f32 takes), 16-byte
 * aligned, ldt and ldte multiples of 4 and >= N; a [B, lda] is read in place from the embedding columns of the builder's xin
 * (a != NULL goes together with E > 0); act: 0 none, 1 tanh.  An index outside [0, I) adds nothing.
 * Order of the sum, per element, all in float32: s = pre (or 0); s += base; s += table[j] for the row's indices in the order
 * they are stored; s = fma(a[b, e], tblE[e], s) for e = 0 .. E-1; s += bias; then act.  One launch, no atomics, no workspace:
 * the same bits on every run.  An empty row gives act(pre + base + embedding terms + bias).                                  */
int gdmcf_gather_fwd_f32(const float* pre, int64_t ldpre, const float* base, const int64_t* indptr, const int32_t* indices,
                         const int64_t* rows, const float* table, int64_t ldt, int I, const float* a, int64_t lda,
                         const float* tblE, int64_t ldte, int E, const float* bias, int act, int B, int N, float* out, int64_t ldo,
                         void* stream);
/* One reverse-diffusion step carried in the first hidden layer's space (START_X target, no sampling noise: between two hidden
 * activations the loop of gaussian_diffusion.py:161-220 is linear in x_t, so p_t = W1x x_t can be stepped instead of x_t):
 *   s[b,n]      = sum_k A[b,k] * M[n,k]
 *   p_next[b,n] = c1[b] * (s[b,n] + v[n]) + c2[b] * p_cur[b,n]      (v NULL: 0)
 *   h_next[b,n] = act(p_next[b,n] + e[n])    (e NULL: 0; act 0 none, 1 tanh; h_next NULL: not written)
 * A [B, lda], M [N, ldm] (K-contiguous, the orientation of an nn.Linear weight), p_cur/p_next/h_next row-major with
 * their own leading dimensions, c1/c2 float32 [B], v/e float32 [N].  p_next may be p_cur.  float32 throughout.
 * A row with c2[b] == 0 does not read p_cur (its p_cur may hold anything).  B, N, K, the leading dimensions and the alignment
 * of every pointer are free: rows that are not 16-byte aligned (or lda / ldm not multiples of 4) take a scalar load path.
 * Order of the sum, per element, all in float32 (v_mfma_f32_16x16x4_f32 = a k-ordered fma chain): K is cut into chunks of 16;
 * chunk c belongs to partial sum c % 4; a partial sum starts at 0 and takes its chunks in ascending order, within a chunk at k0
 * the terms k0 + j + 4 q for j = 0..3 (outer), q = 0..3 (inner), each by one fma; then s = ((s_0 + s_1) + s_2) + s_3;
 * t = s + v; p_next = fma(c2, p_cur, c1 * t); h_next = act(p_next + e).  One launch, no atomics, no host synchronisation
 * (capture-safe): the same bits on every run.  The four partial sums meet in LDS, so no workspace is needed:
 * gdmcf_latent_step_ws_bytes returns 0 and `ws` may be NULL (the arguments are kept for a later split over workgroups).    */
int gdmcf_latent_step_f32(const float* A, int64_t lda, const float* M, int64_t ldm, const float* v,
                          const float* p_cur, int64_t ldpc, const float* c1, const float* c2, const float* e, int act,
                          int B, int N, int K, float* p_next, int64_t ldpn, float* h_next, int64_t ldh,
                          void* ws, size_t ws_bytes, void* stream);
size_t gdmcf_latent_step_ws_bytes(int B, int N, int K);
/* gdmcf_latent_step_f32 with two optional parts, for the loops that are linear in x_t but not covered by the plain step (the
 * EPSILON target, DNNCat):
 *   row addend   r [B, ldr] (NULL: none):  h_next[b,n] = act((p_next[b,n] + r[b,n]) + e[n])  -- in this order, every sum rounded
 *                to float32; p_next itself is stored without r.  16-byte loads where r and ldr allow, scalars otherwise (as e).
 *   accumulator  q_next [B, ldqn] (NULL: none; then q_cur / qa / qb are not read), q_cur [B, ldqc], qa, qb float32 [B]:
 *                  q_next[b,k] = fma(qa[b], q_cur[b,k], qb[b] * A[b,k])      for k < K
 *                (the product qb * A rounded, then one fma).  A row with qa[b] == 0 does not read q_cur.  q_next may be q_cur,
 *                never A (other workgroups still read A).  Columns k >= K of q_next are not written.  Every element is written
 *                exactly once, with plain stores, by the workgroup that holds it as an operand: no further load of A.
 * With r == NULL and q_next == NULL, p_next and h_next are gdmcf_latent_step_f32's bit for bit (same sums, same order); that
 * entry's own kernel is unchanged.  One launch, no atomics, no workspace (ws may be NULL), no host synchronisation.             */
int gdmcf_latent_step_ex_f32(const float* A, int64_t lda, const float* M, int64_t ldm, const float* v,
                             const float* p_cur, int64_t ldpc, const float* c1, const float* c2, const float* r, int64_t ldr,
                             const float* e, int act, int B, int N, int K, float* p_next, int64_t ldpn, float* h_next,
                             int64_t ldh, const float* q_cur, int64_t ldqc, const float* qa, const float* qb, float* q_next,
                             int64_t ldqn, void* ws, size_t ws_bytes, void* stream);
/* The accumulator of gdmcf_latent_step_ex_f32 as a launch of its own (the last step of a loop, where no step kernel runs):
 *   q_next[b,k] = fma(qa[b], q_cur[b,k], qb[b] * A[b,k])   for k < K -- the same expression, the same bits.
 * All pointers required; lda, ldqc, ldqn >= K; q_next may be q_cur, never A; a row with qa[b] == 0 does not read q_cur.      */
int gdmcf_latent_acc_f32(const float* q_cur, int64_t ldqc, const float* qa, const float* A, int64_t lda, const float* qb,
                         int B, int K, float* q_next, int64_t ldqn, void* stream);
/* Last layer fused with the per-row diffusion loss (gaussian_diffusion.py:335 mean_flat):
 *   out = A @ W^T + bias ;  diff[m,n] = alpha[m]*out[m,n] - target[m,n]   (alpha NULL -> 1)
 *   rowsum[m] = sum_n diff[m,n]^2  (deterministic two-stage reduction)
 * `out` may be NULL (training never needs it).  rowpart: scratch [M, gdmcf_loss_tiles(N)].  rowsum NULL: the second stage is
 * left to the caller (gdmcf_linear_bwd_input_tail_f32). */
int gdmcf_loss_tiles(int N);
int gdmcf_linear_loss_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw,
                              const float* bias, const float* target, int64_t ldt,
                              const float* alpha, int M, int N, int K, float* out, int64_t ldo,
                              float* diff, int64_t ldd, float* rowpart, float* rowsum,
                              void* stream);
/* The same product with the target given as BITMAPS of {0,1} rows (word n>>5 of row m, bit n&31; row stride ldbits words)
 * instead of a dense float matrix: the CSR input path (gdmcf_dnn_prep_input_csr_f32 writes the bitmaps) never densifies
 * the batch.  x0-target training only (the eps target is the noise); results are bit-identical to the dense entry.    */
int gdmcf_linear_loss_fwd_bits_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                   const uint32_t* target_bits, int64_t ldbits, const float* alpha, int M, int N, int K,
                                   float* out, int64_t ldo, float* diff, int64_t ldd, float* rowpart, float* rowsum,
                                   void* stream);
/* Last layer fused with the reverse-diffusion posterior mean (gaussian_diffusion.py:473-515,
 * :451-471, :518-523, :210-217):  out = A @ W^T + bias
 *   pred = eps_mode ? r1[t]*x_t - r2[t]*out : out ;  mean = c1[t]*pred + c2[t]*x_t
 *   x_next = mean + (t!=0 ? sigma[t]*z : 0)            (z NULL -> deterministic)
 * per-row coefficient vectors c1,c2,r1,r2,sigma are float32 [M] (already gathered by t).    */
int gdmcf_linear_posterior_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw,
                                   const float* bias, const float* x_t, int64_t ldxt,
                                   const float* c1, const float* c2, const float* r1,
                                   const float* r2, const float* sigma, const float* z,
                                   int64_t ldz, int M, int N, int K, float* x_next,
                                   int64_t ldxn, float* pred_out, int64_t ldp, void* stream);
/* dA[M,K] = rowscale[m] * (dZ[M,N] @ W[N,K]) * (act==1 ? 1 - Aact[m,k]^2 : 1)
 * (grad wrt the layer input, fused with the previous layer's tanh').  rowscale may be NULL. */
int gdmcf_linear_bwd_input_f32(const float* dZ, int64_t lddz, const float* W, int64_t ldw,
                               const float* rowscale, const float* Aact, int64_t ldact, int act,
                               int M, int N, int K, float* dA, int64_t ldda, void* ws,
                               size_t ws_bytes, void* stream);
/* The input gradient of the LAST layer of a training step together with the step's three small launches that stand between the
 * loss product and it -- none of which writes anything the product reads:
 *   (1) rowsum[m] = sum_j rowpart[m, j], j < nt       what gdmcf_linear_loss_fwd_*_f32 runs behind its product unless its
 *                                                      rowsum is NULL (then gdmcf_loss_parts_last() is nt)
 *   (2) gdmcf_row_loss_finish_mean_f64 on that rowsum  (B = M; T, H, the history and every output as there)
 *   (3) gdmcf_rowscale_f32(A, lda, rowscale, M, Ka, out, ldo)   rowscale is usually (2)'s rowscale_mean
 * The entry then runs gdmcf_linear_bwd_input_f32 with the arguments in front of `tail`; its `rowscale` may be written by (2).
 * Where the register-streaming kernel (family 5) takes the product and its task list leaves a workgroup without work, that one
 * workgroup runs (1)-(3) in this order INSIDE the product's launch, on a compute unit the product does not use; otherwise --
 * product not taken, GDMCF_DR_KN=0, no idle workgroup, more LDS than (2) may have, GDMCF_KN_TAIL=0 -- (1), (2), (3) are
 * launched on their own and gdmcf_linear_bwd_input_f32 after them.  Every buffer holds the same bits either way, and
 * gdmcf_debug_last_gemm reports what the plain entry would.  All pointers of (1)-(3) as their own entries require them. */
typedef struct GdKnTail {
    const float* rowpart;
    int ld_rowpart, nt;
    float* rowsum;
    const float* rowdiv;
    const float* alpha;
    const int64_t* ts;
    const double* weight_t;
    const double* pt;
    int T, H;
    double* Lt_history;
    int64_t* Lt_count;
    int update_history;
    double* loss_unscaled;
    double* loss;
    float* gradcoef;
    double* loss_mean;
    float* rowscale_mean;
    const float* A;
    int64_t lda;
    const float* rowscale;
    int Ka;
    float* out;
    int64_t ldo;
} GdKnTail;
int gdmcf_linear_bwd_input_tail_f32(const float* dZ, int64_t lddz, const float* W, int64_t ldw, const float* rowscale,
                                    const float* Aact, int64_t ldact, int act, int M, int N, int K, float* dA, int64_t ldda,
                                    void* ws, size_t ws_bytes, const GdKnTail* tail, void* stream);
/* (1), (2), (3) of a tail job over M rows as three launches of their own: what gdmcf_linear_bwd_input_tail_f32 issues where the
 * job cannot ride, for a caller whose step does not reach that entry. */
int gdmcf_kn_tail_run(const GdKnTail* tail, int M, void* stream);
/* Partial row sums per row (nt above) that the calling thread's last gdmcf_linear_loss_fwd_f32 / _bits_f32 product wrote. */
int gdmcf_loss_parts_last(void);
/* 1 when the register-streaming kernel, on the current device, would take the product C[M, N] with reduction length K (the input
 * gradient dZ[M, K] W[K, N]) AND leave a workgroup without work for a tail job; host only, nothing launched.  The call itself may
 * still decline (alignment, workspace, the switches). */
int gdmcf_debug_kn_tail_rides(int M, int N, int K);
/* dW[N,K] = dZ[M,N]^T @ A[M,K]  (weight grad; accumulate != 0 adds into dW)
 * db[N]   = sum_m rowscale[m]*dZ[m,n]   (db NULL -> skipped).  When rowscale != NULL the
 * caller passes A already multiplied by rowscale (see gdmcf_rowscale_f32).
 * a_scale_col != 0 is the caller's statement that lda > K and A[m, K] == rowscale[m] for every
 * row m (== 1 when rowscale is NULL) -- which is how gdmcf_rowscale_f32 leaves its output when
 * ldo > K, and how gdmcf_dnn_prep_input_*_f32 leave xin (column I + E holds 1 when ldxin > I + E):
 * db then comes out of the product as its column K (no second pass over dZ).  The library keeps NO record between
 * calls and does not check the column; with a_scale_col == 0 (any A, any column K) db takes a
 * column-sum pass over dZ -- the same result within float32 rounding.  Kernels that cannot
 * carry the extra column (bf16 / f32x3 modes, small shapes) ignore the flag and take the pass. */
int gdmcf_linear_bwd_weight_f32(const float* dZ, int64_t lddz, const float* A, int64_t lda,
                                const float* rowscale, int a_scale_col, int M, int N, int K,
                                float* dW, int64_t lddw, float* db, int accumulate, void* stream);
/* Weight gradient fused with the AdamW update of that weight (single-GPU optimiser-in-backward):
 * G = dZ^T @ A stays in the MFMA accumulators and W, exp_avg, exp_avg_sq ([N,K], row stride ldw, all three) are
 * updated in the epilogue with torch.optim.AdamW's single-tensor math for step number `step`
 * (32 -> 24 B/param of HBM traffic; the gradient is never materialised).  W must not be read by later
 * kernels of the same backward pass (the caller computes the input gradient first).  a_scale_col: as above. */
int gdmcf_linear_bwd_weight_adamw_f32(const float* dZ, int64_t lddz, const float* A, int64_t lda,
                                      const float* rowscale, int a_scale_col, int M, int N, int K, float* W,
                                      int64_t ldw, float* exp_avg, float* exp_avg_sq, float* db, float lr,
                                      float beta1, float beta2, float eps, float weight_decay, int step,
                                      float grad_scale, void* stream);
/* The arguments of one gdmcf_linear_bwd_weight_adamw_f32 call, for the list form below. */
typedef struct GdDwAdamw {
    const float* dZ;
    int64_t lddz;
    const float* A;
    int64_t lda;
    const float* rowscale;
    int a_scale_col, M, N, K;
    float* W;
    int64_t ldw;
    float* exp_avg;
    float* exp_avg_sq;
    float* db;
    float lr, beta1, beta2, eps, weight_decay;
    int step;
    float grad_scale;
} GdDwAdamw;
/* n such products, each with the contract of gdmcf_linear_bwd_weight_adamw_f32 and the same results bit for bit, issued as
 * ONE kernel launch when the register-streaming kernel takes all of them (f32 mode, the same reduction length M, at most 4
 * per launch; longer lists go in groups of 4), else as n consecutive calls of the single entry.  One launch pays the ramp,
 * the final optimiser-stream drain and the ragged last round of tiles once instead of once per weight.  No W of the list
 * may be read by later kernels of the same backward pass, nor be an operand (dZ, A) of another entry; the entries'
 * W / exp_avg / exp_avg_sq / db must not overlap. */
int gdmcf_linear_bwd_weight_adamw_multi_f32(const GdDwAdamw* list, int n, void* stream);
/* out[m, k] = rowscale[m] * A[m, k], k < K (the scaled activation copy of the weight-gradient product: (rs . dZ)^T A ==
 * dZ^T (rs . A)); with ldo > K also out[m, K] = rowscale[m]: the column gdmcf_linear_bwd_weight_*'s a_scale_col speaks of. */
int gdmcf_rowscale_f32(const float* A, int64_t lda, const float* rowscale, int M, int K, float* out,
                       int64_t ldo, void* stream);
/* ---- pieces of the indexIn backbone DNNOneHotEmbedding (models/DNN.py:510-682) ----------------
 * Its output layer is a cosine similarity (:655, :667-682): scores = (u @ V^T) / (|u| |v|^T) with u = [h, h_U,
 * embedding_user(index)] and V = embedding_item.weight.  The products run on gdmcf_linear_* with the row-normalised
 * operands (gdmcf_rowscale_f32 by the inverse norms); these entries are the HBM-bound glue around them:
 *   row_norms:          norm[r] = |X[r,:]|, inv_norm[r] = 1/|X[r,:]|                     (torch.norm(dim=1), :675-676)
 *   normalize_rows_bwd: dX = (dY - Y * <dY, Y>) * inv_norm for Y = X/|X| (backward of the division; dX may alias dY)
 *   tanh_bwd:           out = (dA + scale[0] * extra) * (1 - A^2)   (tanh' of the two hidden activations whose
 *                       gradient also receives the NT-Xent term's, DNN.py:641-643; extra NULL -> no addend;
 *                       scale is a device scalar)
 *   gather_rows:        dst[j,:] = src[index[j],:]                                        (nn.Embedding lookup, :650)
 *   scatter_add_rows:   dst[index[j],:] += src[j,:]                                       (its backward)            */
int gdmcf_row_norms_f32(const float* X, int64_t ld, int rows, int cols, float* norm, float* inv_norm,
                        void* stream);
int gdmcf_normalize_rows_bwd_f32(const float* dY, int64_t lddy, const float* Y, int64_t ldy,
                                 const float* inv_norm, int rows, int cols, float* dX, int64_t lddx,
                                 void* stream);
int gdmcf_tanh_bwd_f32(const float* dA, int64_t ldd, const float* A, int64_t lda, const float* extra,
                       int64_t lde, const float* scale, int M, int N, float* out, int64_t ldo,
                       void* stream);
int gdmcf_gather_rows_f32(const float* src, int64_t lds, const int64_t* index, int n, int cols, float* dst,
                          int64_t ldd, void* stream);
int gdmcf_scatter_add_rows_f32(const float* src, int64_t lds, const int64_t* index, int n, int cols,
                               float* dst, int64_t ldd, void* stream);
/* Optimiser-in-backward for the two embedding tables of the indexIn backbones (FusedAdamW.fuse_into_backward).  Both
 * apply torch.optim.AdamW's single-tensor math for step number `step` -- the element function, scalars and grad_scale
 * of gdmcf_adamw_f32 / gdmcf_linear_bwd_weight_adamw_f32 -- to a table whose gradient is never materialised; the
 * table and its moments share one row stride (ldx / ldw).  Results are bit-identical to the two-pass sequences named.
 *   normalize_rows_bwd_adamw: the gradient of X is normalize_rows_bwd's dX (same reduction order) for Y = X/|X|:
 *                       X, exp_avg, exp_avg_sq updated in one pass (== normalize_rows_bwd into a buffer, then
 *                       gdmcf_adamw_f32).  dY, Y, inv_norm must not alias X or the moments.
 *   scatter_rows_adamw: every one of the `rows` rows of W is updated; row index[j] (j < n) with gradient src[j, :],
 *                       every other row with gradient 0 (== zero a dense gradient, gdmcf_scatter_add_rows_f32 into it,
 *                       then gdmcf_adamw_f32).  The ids of one call must be distinct (as scatter_add_rows assumes);
 *                       ids outside [0, rows) are ignored.  n == 0: every row takes gradient 0. */
int gdmcf_normalize_rows_bwd_adamw_f32(const float* dY, int64_t lddy, const float* Y, int64_t ldy,
                                       const float* inv_norm, int rows, int cols, float* X, int64_t ldx,
                                       float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                                       float eps, float weight_decay, int step, float grad_scale, void* stream);
int gdmcf_scatter_rows_adamw_f32(const float* src, int64_t lds, const int64_t* index, int n, int rows, int cols,
                                 float* W, int64_t ldw, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 void* stream);
/* Gradients of the timestep-embedding branch (models/DNN.py:73-74,78):
 *   demb[m,e] = sum_n dZ1[m,n]*W1[n, I+e] ;  dWe = demb^T @ temb ;  dbe = sum_m demb
 * demb_ws: float32 scratch of (M + N) * E elements.  dWe [E, E] and dbe [E] are overwritten, not
 * accumulated into.  No pointer is optional (GDMCF_E_ARG for a NULL); I >= 0.                 */
int gdmcf_emb_bwd_f32(const float* dZ1, int64_t lddz, const float* W1, int64_t ldw, int I, int E,
                      const float* temb, int M, int N, float* demb_ws, float* dWe, float* dbe,
                      void* stream);

/* ---- per-row loss tail, float64 (gaussian_diffusion.py:339-370) --------------------------
 *   loss[b] = weight_t[ts[b]] * (float64)(rowsum[b]/rowdiv[b]) ; Lt-history FIFO update in
 *   batch order (:355-368) ; loss[b] /= pt[b].   rowdiv = I (mse) or 2I (likelihood), f32.
 * weight_t: float64 [T].  pt: float64 [B].  Lt_history: float64 [T,H]; Lt_count: int64 [T].
 * gradcoef[b] (optional) = d loss[b] / d out[b,n] / diff[b,n] = 2*alpha[b]*weight/(pt*rowdiv),
 * the per-row factor the backward multiplies `diff` by (alpha NULL -> 1).
 * update_history == 0 leaves the ring buffer untouched (data-parallel ranks call
 * gdmcf_lt_history_update on the gathered batch instead).
 * Optional pointers (NULL allowed): alpha, gradcoef, and Lt_history / Lt_count when update_history == 0.  Every other
 * pointer is required (GDMCF_E_ARG for a NULL).  ts must lie in [0, T): it is not checked.    */
int gdmcf_row_loss_finish_f64(const float* rowsum, const float* rowdiv, const float* alpha,
                              const int64_t* ts, const double* weight_t, const double* pt, int B,
                              int T, int H, double* Lt_history, int64_t* Lt_count,
                              int update_history, double* loss_unscaled, double* loss,
                              float* gradcoef, void* stream);
/* The same tail, additionally emitting what the reference's step computes next (main.py:348-350): loss_mean (optional,
 * float64 scalar) = mean_b loss[b], summed in a fixed order, and rowscale_mean[b] (optional, float32) = gradcoef[b] *
 * (float)(1/B) -- the per-row scale of the backward of that mean -- so that the step needs no reduction / scaling launch.
 * loss_mean and rowscale_mean are optional like alpha and gradcoef above; rowscale_mean needs gradcoef (GDMCF_E_ARG without).
 * gdmcf_lt_history_update has no optional pointer. */
int gdmcf_row_loss_finish_mean_f64(const float* rowsum, const float* rowdiv, const float* alpha, const int64_t* ts,
                                   const double* weight_t, const double* pt, int B, int T, int H, double* Lt_history,
                                   int64_t* Lt_count, int update_history, double* loss_unscaled, double* loss,
                                   float* gradcoef, double* loss_mean, float* rowscale_mean, void* stream);
int gdmcf_lt_history_update(const int64_t* ts, const double* loss_unscaled, int B, int T, int H,
                            double* Lt_history, int64_t* Lt_count, void* stream);

/* ---- data-parallel exchange helpers (new: the reference is single-process; main.py:345-351 is the step whose
 * gradients are exchanged).  One float64 buffer `flat` carries, per rank and step,
 *   [ sum(counts) ]   the n (<= 16) small float32 gradients, concatenated in table order, and
 *   [world][B][2]     (ts, unscaled loss) of every rank's rows -- a rank writes its own slice, zeros elsewhere,
 * so a single SUM all-reduce of `flat` both reduces the small gradients and gathers the history inputs in rank
 * order (what gdmcf_lt_history_update then replays on the global batch).  `grads` / `counts` are HOST arrays of
 * device pointers / element counts (copied into the kernel arguments).
 * pack: flat <- this rank's contribution.  unpack: gradients <- (float)flat, ts_all[world*B] (int64) and
 * loss_unscaled_all[world*B] (float64) contiguous in rank order.                                              */
int gdmcf_dp_pack_f64(const float* const* grads, const int64_t* counts, int n, const int64_t* ts,
                      const double* loss_unscaled, int B, int rank, int world, double* flat,
                      void* stream);
int gdmcf_dp_unpack_f64(const double* flat, float* const* grads, const int64_t* counts, int n, int B,
                        int world, int64_t* ts_all, double* loss_unscaled_all, void* stream);

/* ---- importance-sampled timesteps (gaussian_diffusion.py:373-397), one launch, no host sync ----
 * Until every Lt_count == H: t ~ uniform{0..T-1}, pt = 1.  Afterwards p = sqrt(mean(Lt_history^2))
 * normalised, mixed as p*(1-uniform_prob) + uniform_prob/T; t by inverse CDF, pt = p[t]*T.
 * Random numbers: Philox4x32-10 (counter (b,0,2,offset), key seed) -- the reference's torch.randint /
 * torch.multinomial streams cannot be reproduced on the device, parity tests inject ts instead.
 * p_out (optional, float64 [T]) receives the probability vector when the importance branch is live. */
int gdmcf_sample_timesteps(const double* Lt_history, const int64_t* Lt_count, int T, int H, int B,
                           double uniform_prob, uint64_t seed, uint64_t offset, int64_t* ts,
                           double* pt, double* p_out, void* stream);

/* ---- fused multi-tensor AdamW (torch.optim.AdamW as used at main.py:258,351) -------------
 * table: device int64 [n_tensors][6] = {param*, grad*, exp_avg*, exp_avg_sq*, numel, first_block}
 * (first_block = prefix sum of ceil(numel/4096)); total_blocks = grid size.
 * grad_scale multiplies every gradient first (1/world_size for data parallel).             */
int gdmcf_adamw_f32(const int64_t* table, int n_tensors, int total_blocks, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, float grad_scale,
                    void* stream);
/* Same update, additionally storing each updated parameter rounded to bfloat16 into its registered shadow:
 * shadow_table [n_tensors][3] int64 device array = (shadow pointer or 0, columns of the 2-D parameter, shadow row
 * stride) as returned by gdmcf_bf16_shadow_info.  Parameters must have fewer than 2^32 elements.              */
int gdmcf_adamw_bf16s_f32(const int64_t* table, const int64_t* shadow_table, int n_tensors, int total_blocks, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                          void* stream);

/* ---- evaluation: history mask + top-k (main.py:296-301) ----------------------------------
 * For every row: entries listed in the CSR history mask become -inf, then the k largest
 * scores are returned in descending order; ties broken by LOWEST index (torch.topk leaves
 * tie order unspecified).  mask_indptr int64 [B+1] / mask_indices int32 (NULL = no mask).  */
int gdmcf_topk_masked_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* mask_indptr,
                          const int32_t* mask_indices, int k, int64_t* idx_out, float* val_out,
                          void* stream);
/* The same selection with the mask picked by row id (gdmcf_amd.recommend): row b of pred is masked by row rows[b] of the FULL
 * CSR (indptr int64 [n_users + 1], indices int32; both NULL = no mask) and, when given, of a second full CSR over the same
 * rows (indptr2 / indices2; needs the first) -- the reference's mask_tv = train + valid without a summed matrix.  rows int64
 * [B], every entry a row of both CSRs (not checked on the device); NULL = rows 0..B-1.  Selection, tie rule (equal scores in
 * ascending item index), degenerate rows (masked items count as -inf and appear, lowest index first, only when fewer than k
 * items are unmasked) and the handling of unsorted, repeated or out-of-range indices are gdmcf_topk_masked_f32's: with
 * scale == NULL idx_out / val_out are bit for bit what it returns for the same pred and the sub-CSR csr[rows] (or
 * (csr + csr2)[rows]).  scale (optional, float32 [B], > 0) multiplies the returned values only, after selection:
 * val_out[b, j] *= scale[b].  Same shape limits and error codes; no global atomics, no workspace, no host synchronisation. */
int gdmcf_topk_masked_rows_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* indptr, const int32_t* indices,
                               const int64_t* indptr2, const int32_t* indices2, const int64_t* rows, const float* scale, int k,
                               int64_t* idx_out, float* val_out, void* stream);
/* The exact position of named items in that order (gdmcf_amd.rank_targets): rank_out[b, j], j < the length of row rows[b] of the
 * target CSR (tgt_indptr int64 [n_users + 1], tgt_indices int32, a FULL CSR like the masks; required), is the number of items
 * i in [0, I) that precede target j -- the 0-based place it would have in gdmcf_topk_masked_rows_f32(..., k = I)'s list for the
 * same pred, masks and rows.  The order is the top-k's: an item's key is the order key of its score, or of -inf when the item
 * occurs in row rows[b] of either mask CSR (indptr / indices, optional indptr2 / indices2 which needs the first; both NULL =
 * no mask; rows unsorted, repeated or out of range as there); larger key first, equal keys in ascending item index; NaN, +-0
 * and +-inf order by the same key map.  A masked target is ranked inside the -inf tail by its index, as the top-k would list
 * it.  A target outside [0, I) gets -1; columns from the row's length up to G get -1; target entries past G are not ranked;
 * columns from G up to ldr are not written.  Target rows may be unsorted and hold repeats: equal targets get equal ranks.
 * rows int64 [B]: the row of EVERY CSR (masks and targets) per pred row, not checked on the device; NULL = rows 0..B-1.
 * n_live_out (optional, int32 [B]): the number of unmasked items of the row, I minus the distinct in-range mask entries --
 * what turns a rank into a percentile or an AUC.
 * Limits: any B >= 1, I >= 1, G >= 1, ldp >= I, ldr >= G (GDMCF_E_SHAPE otherwise).  Targets are ranked in passes of up to 1024
 * (the row is streamed once per pass; one pass for G <= 1024), fewer per pass where the mask bitmap of I bits leaves less
 * room: the plan -- 12 bytes per target of a pass plus I / 8 bytes -- must fit 160 KiB of LDS with 32 targets a pass, so I up
 * to about 1.3 million, the width gdmcf_topk_masked_rows_f32 takes; wider rows return GDMCF_E_UNSUPPORTED.
 * The counts are integers added by LDS atomics: the same result in every run.  No global atomics, no workspace, no host
 * synchronisation.                                                                                                      */
int gdmcf_rank_targets_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* indptr, const int32_t* indices,
                           const int64_t* indptr2, const int32_t* indices2, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                           const int64_t* rows, int G, int32_t* rank_out, int64_t ldr, int32_t* n_live_out, void* stream);

/* ---- candidate lists: score only the items a caller names (gdmcf_amd.score_candidates, recommend(candidates=)) -----------
 * The gathered product: out[b, c] = (dot(A[b, :K], W[cand[b, c], :K]) + bias[cand[b, c]]) * scale[b] for b < B, c < C -- the
 * last product of a latent reverse loop (engine_core.LatentProduct) on the rows of W a list names, instead of all I of them.
 * A [B, lda >= K]; W [I, ldw >= K], rows K-contiguous; bias [I] or NULL; scale float32 [B] or NULL (no multiplication);
 * cand int64 [B, ldcand >= C], or ldcand == 0: one list [C] shared by all rows; out [B, ldo >= C].  1 <= K <= 4096, any
 * B >= 1, C >= 1 (GDMCF_E_SHAPE otherwise).  Mask arguments as gdmcf_topk_masked_rows_f32's (indptr / indices, optional
 * indptr2 / indices2, rows or NULL = rows 0..B-1): a candidate that occurs in row rows[b] of either CSR gets -inf; the rows
 * may be unsorted and hold repeats and out-of-range entries.  A candidate outside [0, I) -- -1, any huge value: the padding of
 * a ragged list -- gets -inf too; for neither kind is a row of W or an element of bias read.  Duplicates are each scored.
 * Summation order, fixed: lane l of a wave adds the products of k = 256 j + 4 l .. + 3 (j ascending, so k ascending) into
 * one accumulator by fma from +0; the 64 accumulators are added in a butterfly over the lane distances 32, 16, 8, 4, 2, 1,
 * x(l) + x(l ^ m) at every level; then (sum + bias) * scale.  The bits of (b, item) depend on neither the item's place in
 * the list, nor C, nor ldcand, nor the run.  No atomics, no workspace, no host synchronisation.                          */
int gdmcf_cand_scores_f32(const float* A, int64_t lda, const float* W, int64_t ldw, int I, int K, const float* bias,
                          const float* scale, const int64_t* cand, int64_t ldcand, int B, int C, const int64_t* indptr,
                          const int32_t* indices, const int64_t* indptr2, const int32_t* indices2, const int64_t* rows, float* out,
                          int64_t ldo, void* stream);
/* The same contract with the score taken from a dense matrix: out[b, c] = dense[b, cand[b, c]] * scale[b] (dense [B, ldd >= I];
 * one float32 multiplication per element, none with scale == NULL), -inf for masked and out-of-range candidates, which are not
 * read.  For every route that already holds [B, I] scores.                                                              */
int gdmcf_cand_pick_f32(const float* dense, int64_t ldd, int B, int I, const float* scale, const int64_t* cand, int64_t ldcand,
                        int C, const int64_t* indptr, const int32_t* indices, const int64_t* indptr2, const int32_t* indices2,
                        const int64_t* rows, float* out, int64_t ldo, void* stream);

/* ---- LightGCN ranking: score product fused with the masked top-k (lightGCN.py:67-127, get_metrics) -----------
 * replaces `relevance_score = user_emb @ item_emb.T`, the dense -inf mask of the training interactions added to it and
 * `torch.topk(relevance_score, K)` (lightGCN.py:75-90) without the [n_rows, n_items] score matrix (nor the mask) ever being
 * stored: row r's scores dot(user_emb[user_ids[r]], item_emb[i]) (float32, v_mfma_f32_16x16x4_f32) are selected from while
 * they are MFMA accumulators.  out_idx [n_rows, k] / out_val [n_rows, k] (optional) are exactly what gdmcf_topk_masked_f32
 * returns for the materialised matrix: descending score, equal scores in ascending item index, the items of row r's mask
 * (CSR over the n_rows rows of the CALL: mask_indptr int64 [n_rows+1], mask_indices int32; NULL = none) count as -inf, so
 * they appear -- lowest index first, value -inf -- only when fewer than k items are unmasked.  user_ids NULL = rows
 * 0..n_rows-1 of user_emb.  Any n_rows, n_items, 1 <= d <= 4096, 1 <= k <= min(n_items, 1024).  Deterministic (same bits
 * from run to run).  ws: gdmcf_score_topk_ws_bytes bytes (k candidates per row and item slab when few rows are asked for; 0
 * when the row tiles fill the chip; never more than 5 % of 4 n_rows n_items).                                            */
size_t gdmcf_score_topk_ws_bytes(int n_rows, int n_items, int d, int k);
int gdmcf_score_topk_f32(const float* user_emb, int64_t ldu, const int64_t* user_ids, int n_rows, const float* item_emb,
                         int64_t ldi, int n_items, int d, const int64_t* mask_indptr, const int32_t* mask_indices, int k,
                         int64_t* out_idx, float* out_val, void* ws, size_t ws_bytes, void* stream);

/* The exact ranks of named items from the same fused product (evaluate_utils.score_rank, LightGCN.rank_targets,
 * lightgcn.get_metrics_at): gdmcf_score_topk_f32's product with the selection replaced by gdmcf_rank_targets_f32's counting, so
 * neither the [n_rows, n_items] score matrix nor a k bounds it.  user_emb / user_ids / item_emb / d and the mask CSR are
 * gdmcf_score_topk_f32's; both CSRs hold one row per ranked row of the CALL (mask_indptr, tgt_indptr int64 [n_rows + 1]; indices
 * int32; the mask optional, the targets required).  Everything else is gdmcf_rank_targets_f32's, so that either entry can stand in
 * for the other: rank_out[r, j] is the number of items that precede target j of row r -- larger key first, equal keys in ascending
 * item index, a masked item carries the key of -inf, a masked target is ranked inside the -inf tail by its index; NaN, +-0 and
 * +-inf order by the same key map.  A target outside [0, n_items) gets -1; columns from the row's length up to G get -1; target
 * entries past G are not ranked; columns from G up to ldr are not written.  Target rows may be unsorted and hold repeats (equal
 * targets get equal ranks); mask rows may be unsorted and hold repeats and out-of-range entries, which are skipped.  n_live_out
 * (optional, int32 [n_rows]): n_items minus the distinct in-range mask entries of the row.
 * A target's own score is formed by the MFMA chain, in the k order, that forms the streamed score of that item (one small launch,
 * one wave per row and 16 targets), so rank_out[r, j] is exactly the place of the item in gdmcf_score_topk_f32's list for the
 * same tables wherever that list reaches.
 * Limits: any n_rows >= 1, n_items >= 1, G >= 1, 1 <= d <= 4096, ldu / ldi >= d, ldr >= G (GDMCF_E_SHAPE; d > 4096 and null or
 * half-given pointers GDMCF_E_ARG; a short, missing or not 16-byte aligned workspace GDMCF_E_WORKSPACE / GDMCF_E_ARG).  Row tiles
 * by G: 64 rows to G = 128, 32 to 256, 16 above, where the targets are ranked in passes of 512 that stream the items again.
 * ws: gdmcf_score_rank_ws_bytes bytes, always needed: 8 bytes per row and target column (G rounded up to 16), 4 bytes per row,
 * pass, item slab and gap (targets of a pass + 1), 4 bytes per row and slab -- it grows with n_rows * G (times the slab count, at
 * most 16 and only when few rows are asked for), never with n_rows * n_items.  Integer sums only: the same bits in every run.
 * gdmcf_debug_score_rank_plan: the plan for a shape (tests pick their G with it): returns 1 and the rows of a tile, the targets
 * of a pass, the passes and the item slabs, or 0 (all four 0) for a shape the entry refuses.                              */
int gdmcf_debug_score_rank_plan(int n_rows, int n_items, int G, int* tile_rows, int* pass_targets, int* passes, int* slabs);
size_t gdmcf_score_rank_ws_bytes(int n_rows, int n_items, int d, int G);
int gdmcf_score_rank_f32(const float* user_emb, int64_t ldu, const int64_t* user_ids, int n_rows, const float* item_emb,
                         int64_t ldi, int n_items, int d, const int64_t* mask_indptr, const int32_t* mask_indices,
                         const int64_t* tgt_indptr, const int32_t* tgt_indices, int G, int32_t* rank_out, int64_t ldr,
                         int32_t* n_live_out, void* ws, size_t ws_bytes, void* stream);

/* Ranking metrics of reference evaluate_utils.py:6-52 (computeTopNAccuracy) on the device: per user and per cut-off
 * N of topN_host (ascending, at most 8) the four terms precision = hits/N, recall = hits/|GT|, NDCG = dcg/idcg,
 * MRR = 1/(rank of the first hit), all 0 for a user with an empty ground truth -- float64, accumulated in rank order
 * exactly as the reference's loop, written to out[U][n_topn][4].  pred_idx: [U, >= max N] item ids (row stride ldp);
 * ground truth as CSR with sorted column indices.  The caller adds the terms up over users and divides by U.        */
int gdmcf_topn_metrics_f64(const int64_t* pred_idx, int64_t ldp, int U, const int64_t* gt_indptr, const int32_t* gt_indices,
                           const int* topN_host, int n_topn, double* out, void* stream);
/* The same four terms from ranks instead of lists: ranks int32 [U, ldr >= G] as gdmcf_rank_targets_f32 writes them for the
 * ground truth as targets (a negative entry = no item there), |GT| = the number of non-negative entries of the row, a hit
 * below N = an entry < N.  The hits are taken in ascending rank and DCG is accumulated in that order, IDCG over
 * j < min(N, |GT|) in ascending j: for ranks that came from a full order the float64 bits equal gdmcf_topn_metrics_f64's on
 * that order's first N items.  A user without entries gets zeros.  topN_host ascending, any values >= 1, at most 8 per call
 * (the host calls it in groups): no list bounds them, a cut-off past the item count counts every hit (recall 1).
 * out[U][n_topn][4].  One wave per user, no atomics: deterministic.                                                     */
int gdmcf_rank_metrics_f64(const int32_t* ranks, int64_t ldr, int U, int G, const int* topN_host, int n_topn, double* out,
                           void* stream);

/* ---- LightGCN propagation: CSR SpMM (lightGCN.py:184-189) --------------------------------
 * Y[r,:] = ( sum_j val[j]*X[col[j],:]  +  sum_k addend_k[r,:] ) * scale
 * The adjacency is plain CSR (col int32, val float32) plus a host-built execution plan of "virtual rows"
 * (gdmcf_amd/spmm_schedule.py:spmm_plan):
 *   vbeg, vend int64 [n_virtual]  nonzero range of each virtual row
 *   vrow  int32 [n_virtual]       the real row it belongs to
 *   vslot int32 [n_virtual]       -1: the row is whole, write Y directly; >= 0: slot in partial_ws
 *   the first n_short virtual rows are WHOLE rows of at most a few dozen nonzeros: they run 64/(d/4) rows per
 *   wave (four at d = 64), because one-row-per-wave is latency bound on such rows;
 *   the remaining ones are pieces of <= chunk nonzeros, one wave each, so hub nodes spread over many waves;
 *   lrow  int32 [n_long], lptr int32 [n_long+1]: the rows that were cut and their slot ranges in
 *   partial_ws float32 [n_slots, d], added up in slot order by a second small kernel (no atomics).
 * With n_short = 0 and chunk = infinity the plan degenerates to plain CSR (vbeg = rowptr[:-1], vend = rowptr[1:]).
 * addends_host: HOST array of n_add (<= 8) device pointers [n_rows, ld_add] -- the last LightGCN
 * layer passes E_0..E_{L-1} and scale = 1/(L+1) so the layer mean (:188-189) costs no extra pass.
 * alg_bytes: algorithmic bytes of this launch, forwarded to the profiling hook only.          */
int gdmcf_spmm_csr_f32(const int64_t* vbeg, const int64_t* vend, const int32_t* vrow, const int32_t* vslot,
                       int n_virtual, int n_short, const int32_t* lrow, const int32_t* lptr, int n_long, const int32_t* col,
                       const float* val, int n_rows, const float* X, int64_t ldx, int d, float* Y,
                       int64_t ldy, float* partial_ws, const float* const* addends_host, int n_add,
                       int64_t ld_add, float scale, double alg_bytes, void* stream);
/* Second-generation schedule of the same product (one launch per layer; csrc/spmm_bundle.hip), for d in
 * {8,16,32,64,128,256} with 16-byte aligned rows.  The host plan (gdmcf_amd/spmm_schedule.py:spmm_bundle_plan) sorts the rows
 * of at most s_max nonzeros by length and bundles them G = 64/(d/4) to a wave-step, cuts longer rows into pieces, and
 * gives every one of n_waves waves (a multiple of 32; block b = 4 waves serves class b % 8 = one XCD) a contiguous run
 * of pieces and bundles of equal cost:
 *   wdesc int32 [n_waves][4]   first / last+1 piece and first / last+1 bundle of the wave (class-major order)
 *   lbeg int64, llen/lrow/lslot int32 [n_pieces]   first nonzero, length, row, partial slot (-1: the row is whole)
 *   sbeg int64, slen/srow int32 [n_bundles*G], smax int32 [n_bundles]   per bundle entry: first nonzero, length, row
 *                                                  (-1 = padding), and the longest length of the bundle
 *   crow int32 [n_cut], cptr int32 [n_cut+1]       rows cut into several pieces and their slot ranges in partial_ws
 * nnz = length of col / val (> 0), n_x_rows = rows of X (columns of the matrix).  Everything else as
 * gdmcf_spmm_csr_f32.  Returns GDMCF_E_UNSUPPORTED for other widths / alignments.               */
int gdmcf_spmm_bundled_f32(const int32_t* wdesc, int n_waves, const int64_t* lbeg, const int32_t* llen, const int32_t* lrow,
                           const int32_t* lslot, int n_pieces, const int64_t* sbeg, const int32_t* slen, const int32_t* srow,
                           const int32_t* smax, int n_bundles, const int32_t* crow, const int32_t* cptr, int n_cut,
                           const int32_t* col, const float* val, int64_t nnz, int n_rows, int n_x_rows, const float* X,
                           int64_t ldx, int d, float* Y, int64_t ldy, float* partial_ws, const float* const* addends_host, int n_add, int64_t ld_add,
                           float scale, double alg_bytes, void* stream);
/* Third generation: the schedule of gdmcf_spmm_bundled_f32 with the nonzeros re-ordered into the order the waves gather
 * them (gdmcf_amd/spmm_schedule.py:spmm_stream_pack), so that a wave reads one contiguous run of (col, val) pairs instead of
 * chasing row pointers:
 *   wdesc int32 [n_waves][4]     first 64-entry batch of the wave's run, its batches, first / last+1 unit
 *   cw    int32 [n_entries][2]   (column, float bits of the value); n_entries % 64 == 0; 8-byte aligned
 *   ud    int32 [n_units][DW]    DW = 1 + max(G, 2), G = 64/(d/4):  [steps/UN | piece << 31,  piece: row, slot (-1 = whole
 *                                row) | bundle: row of lane group g (-1 = padding, bit 30 = empty row)], UN = min(4, d/4)
 *   crow / cptr / partial_ws / addends / scale / alg_bytes as above.                                                     */
int gdmcf_spmm_stream_f32(const int32_t* wdesc, int n_waves, const int32_t* cw, int64_t n_entries, const int32_t* ud, int n_units,
                          const int32_t* crow, const int32_t* cptr, int n_cut, int n_rows, int n_x_rows, const float* X,
                          int64_t ldx, int d, float* Y, int64_t ldy, float* partial_ws, const float* const* addends_host,
                          int n_add, int64_t ld_add, float scale, double alg_bytes, void* stream);
/* development aid (tools/spmm_waves.py): per-wave timestamps of gdmcf_spmm_stream_f32's main kernel.  (n_waves, NULL) starts
 * recording 8 int64 per wave -- start, first gather, end of pieces, end (100 MHz ticks), units, batches, XCC id, block --,
 * (n_waves, host buffer) copies them out and stops.                                                                     */
int gdmcf_debug_spmm_stamps(int n_waves, long long* host_out);
/* ---- graph step state: what changes from step to step, in device memory (hipGraph replay freezes kernel arguments) ----
 * A training step captured in a hipGraph (gdmcf_amd/graph.py) replays the SAME launches; the Philox offsets of the input
 * builder / timestep sampler and the AdamW bias corrections therefore come from a device block (opaque,
 * gdmcf_graph_state_bytes() bytes, filled on the host by gdmcf_graph_state_init and copied to the device by the caller)
 * that gdmcf_graph_state_tick advances by one step: offsets + 1, optimiser step + 1, scalars of that step taken from a
 * host-computed table (gdmcf_adam_hyper_fill: n entries of gdmcf_adam_hyper_bytes() bytes for steps first_step ..., the
 * same double-precision formulas as gdmcf_adamw_f32 -> bit-identical updates).  While a block is bound to the calling
 * thread (gdmcf_graph_state_bind; NULL unbinds) gdmcf_dnn_prep_input(_csr)_f32, gdmcf_sample_timesteps and gdmcf_adamw_*
 * ignore their offset / step arguments and read the block instead.                                                      */
int gdmcf_graph_state_bytes(void);
int gdmcf_adam_hyper_bytes(void);
int gdmcf_graph_state_init(void* state_host, uint64_t prep_offset, uint64_t ts_offset, int64_t adam_step, int64_t table_first,
                           int64_t table_len, const void* hyper_table_dev);
int gdmcf_adam_hyper_fill(void* out_host, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int64_t first_step, float grad_scale);
int gdmcf_graph_state_bind(const void* state_dev);
int gdmcf_graph_state_tick(void* state_dev, void* stream);
/* out = acc * scale, n > 0 elements; both pointers are required (GDMCF_E_ARG for a NULL) */
int gdmcf_scale_f32(const float* acc, int64_t n, float scale, float* out, void* stream);

/* ---- LightGCN BPR training step (lightGCN.py:207-251, :287-300; csrc/bpr.hip) -------------------------------------------
 * Notation: M [N, d] the propagated mean table, E0 [N, d] the parameter, N = n_users + n_items, item i = node n_users + i,
 * B triples (users[j], pos[j], neg[j]) of int64 ids (pos / neg are ITEM ids), x_j = <M[u_j], M[neg_j]> - <M[u_j], M[pos_j]>.
 * No float atomics anywhere: same inputs, same bits.
 *
 * gdmcf_bpr_sample_f32 replaces the reference's per-user `random.choice(x)` / `sample_neg(x)` (lightGCN.py:225-229,
 * :244-246): for each users[j] one interacted and one non-interacted item of the training CSR (indptr int64 [n_users+1],
 * indices int32, every row sorted and free of duplicates), one thread per triple, Philox4x32-10 with counter
 * (j, 0, 7, offset) and key seed -- stream id 7.  pos[j] is uniform over the row; neg[j] is uniform over the
 * n_items - deg items NOT in the row, drawn exactly (no rejection loop): r uniform in [0, n_items - deg), i = the smallest
 * index with row[i] - i > r (binary search; i = deg when there is none), neg = r + i -- the distribution of sample_neg.
 * Integers come from 32-bit words by multiply-high, floor(w n / 2^32): the bias of any outcome is at most n / 2^32.
 * A user outside [0, n_users), or with deg == 0 or deg == n_items, gets pos = neg = -1 and *flag (int32, optional) = 1.   */
int gdmcf_bpr_sample_f32(const int64_t* indptr, const int32_t* indices, const int64_t* users, int B, int n_users, int n_items,
                         uint64_t seed, uint64_t offset, int64_t* pos, int64_t* neg, int32_t* flag, void* stream);
/* gdmcf_bpr_sample_pool_f32 generalises that draw (lightGCN.py:225-246) to n_negs negatives per positive, each the
 * best-scored of `pool` candidates under the propagated table M [n_users + n_items, ldm] (dynamic negative sampling).
 * pos [B] as above: row[mulhi(x, deg)], x the first word of the block with counter (j, 0, 7, offset).  neg [B * n_negs],
 * neg[j * n_negs + k] = the negative of slot k.  Candidate q = k * pool + c of triple j (pool position c) is the
 * mulhi(w_q, n_items - deg)-th item missing from the row (the same binary search); w_q is word y, z, w of block 0 for
 * q = 0, 1, 2 and word (q - 3) % 4 of the block with counter (j, 1 + (q - 3) / 4, 7, offset) for q >= 3, so
 * n_negs = pool = 1 is gdmcf_bpr_sample_f32 bit for bit.  Candidates are independent: repeats inside a pool and between
 * slots are allowed.  pool == 1: the candidate is the negative and M is not read (M may be NULL).  pool > 1: the score of
 * candidate i is the float32 dot product <M[users[j]], M[n_users + i]>; the slot keeps its first candidate unless a later
 * one scores strictly greater (equal scores keep the earliest drawn; a NaN score never replaces anything).  One lane group
 * per slot (j, k) as gdmcf_bpr_loss_f32, one thread per slot at pool == 1; no atomics.  A user outside [0, n_users), or
 * with deg == 0 or deg == n_items, gets pos = -1, all n_negs negatives -1 and *flag (int32, optional) = 1.
 * E_SHAPE: B, n_negs or pool < 1, n_negs * pool >= 2^20, d < 1 or ldm < d with M given; E_ARG: a null pointer, M == NULL
 * with pool > 1.                                                                                                         */
int gdmcf_bpr_sample_pool_f32(const int64_t* indptr, const int32_t* indices, const int64_t* users, int B, int n_negs, int pool,
                              int n_users, int n_items, const float* M, int64_t ldm, int d, uint64_t seed, uint64_t offset,
                              int64_t* pos, int64_t* neg, int32_t* flag, void* stream);
/* gdmcf_bpr_loss_f32 replaces the six row gathers of LightGCN.forward (lightGCN.py:200-201) and bpr_loss (:207-219):
 *   coef[j] = sigmoid(x_j) / B           the derivative of mean_j softplus(x_j) (torch's softplus: linear above 20)
 *   *mf     = mean_j softplus(x_j)
 *   *reg    = 0.5 (sum_j |E0[u_j]|^2 + |E0[pos_j]|^2 + |E0[neg_j]|^2) / B
 * One lane group per triple (16 lanes x float4 at d = 64), then ONE fixed-order reduction of the per-triple partials in
 * ws (float [2 B]).  Any d >= 1 (float4 loads when d % 4 == 0 and the rows are 16-byte aligned).  A triple with an id out
 * of range contributes nothing, gets coef 0 and sets *flag (int32, optional) = 1.                                        */
int gdmcf_bpr_loss_f32(const float* M, int64_t ldm, const float* E0, int64_t lde, int d, const int64_t* users, const int64_t* pos,
                       const int64_t* neg, int B, int n_users, int n_items, float* coef, float* ws, float* mf, float* reg,
                       int32_t* flag, void* stream);
/* gdmcf_bpr_grad_f32 replaces what autograd runs behind `final_loss.backward()` (lightGCN.py:299) up to the propagation:
 * the six index_put_(accumulate) scatters into zeroed tables.  Entry e in [0, 3 B) of the batch is (role e / B: 0 user,
 * 1 pos, 2 neg; triple e % B); order int32 [3 B] lists the entries sorted by node, entries of one node in ascending e.
 * One lane group per entry; the first entry of a node's run walks the run and is the row's only writer.
 *   mode 0: out[node] = sum over the run of  user: coef_j (src[neg_j] - src[pos_j]),  pos: -coef_j src[u_j],
 *           neg: +coef_j src[u_j]   with src = M: the cotangent of the propagated table.  Rows of no entry are not written.
 *   mode 1: out[node] += scale * (entries in the run) * src[node]   with src = E0, scale = decay / B: the regulariser's
 *           gradient, added to the propagated cotangent; zero_rows (optional, [N, ld_zero]): row node of it is cleared
 *           in the same pass (a persistent cotangent table is all zero again afterwards).                                 */
int gdmcf_bpr_grad_f32(int mode, const int32_t* order, const int64_t* users, const int64_t* pos, const int64_t* neg, int B,
                       int n_users, int n_items, const float* coef, const float* src, int64_t ld_src, int d, float* out,
                       int64_t ld_out, float scale, float* zero_rows, int64_t ld_zero, void* stream);

/* ---- DNNCat backbone: the cat layer in front of the plain DNN (models/DNN.py:180-265; csrc/cat.hip) ----------------------
 * cat_w [3] / cat_b [1] are cat_layer's parameters IN DEVICE MEMORY (the optimiser moves them every step: no host read, no
 * sync).  xU [B, ldu] is the one-hot image of gdmcf_onehot_noise_f32 (item i in columns 2i, 2i + 1).
 *
 * gdmcf_cat_prep_input_f32 replaces q_sample (gaussian_diffusion.py:399-407), `torch.cat([x.unsqueeze(-1), x_U], dim=2)`,
 * `cat_layer(x).squeeze()`, `self.drop(x)` and `torch.cat([x, emb], dim=-1)` of DNNCat.forward (models/DNN.py:244-255; the
 * timestep embedding of :245-246 through gdmcf_dnn_emb_cols_f32, launched from here) -- one pass over [B, I]:
 *   x_t  = ca[ts[b]] x0 + cb[ts[b]] noise     as gdmcf_dnn_prep_input_f32 forms it, bit for bit (same noise_mode, Philox
 *                                             counters and Box-Muller); ca == NULL: x_t = x0
 *   z    = ((w0 x_t + w1 xU[b,2i]) + w2 xU[b,2i+1]) + c      float32, every operation rounded, no fused multiply-add
 *   xin[b, 0:I] = dropout(z)                  drop_mode 0 none / 1 keep [B, ldkeep] uint8 / 2 Philox stream 1 with the plain
 *                                             builder's counters; kept values times 1/(1-p)
 *   xin[b, I:ldxin] = [ emb(t) | 1 | 0-pad ]  the layout of gdmcf_dnn_prep_input_f32;  temb_out [B, E] as there
 *   xt_out[b, 0:I] = x_t                      all the backward pass keeps (the drawn keep-mask is recomputed there)
 * E > 0; xin and xt_out 16-byte aligned with leading dimensions that are multiples of 4.                                  */
int gdmcf_cat_prep_input_f32(const float* x, int64_t ldx, const float* xU, int64_t ldu, const int64_t* ts, const float* ca,
                             const float* cb, int noise_mode, const float* noise, int64_t ldn, int drop_mode, const uint8_t* keep,
                             int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, const float* cat_w, const float* cat_b,
                             const float* emb_w, const float* emb_b, int E, int B, int I, float* xin, int64_t ldxin, float* xt_out,
                             int64_t ldxt, float* temb_out, void* stream);
/* gdmcf_cat_grad_f32 replaces what autograd runs behind the dropout and cat_layer of models/DNN.py:248-253: with
 * dxin [B, I] = dZ1 . W1[:, 0:I] (gdmcf_linear_bwd_input_f32 on the first I columns of the first layer's weight) and
 * dz = dxin * keep / (1-p) -- drop_mode / keep / drop_p / seed / offset as given to gdmcf_cat_prep_input_f32 --
 *   grad_w[0..2] = (sum dz x_t, sum dz xU[.,2i], sum dz xU[.,2i+1]),   grad_b[0] = sum dz        over all b, i.
 * Two stages, no atomics (same inputs, same bits): float32 partials per workgroup of 4096 columns of a row (wave shuffles and
 * one LDS exchange) in ws (gdmcf_cat_grad_ws_bytes(B, I) bytes, 16-byte aligned), then one workgroup adds the partials in
 * index order in float64 and rounds once.  grad_w / grad_b are device pointers and are OVERWRITTEN.                        */
size_t gdmcf_cat_grad_ws_bytes(int B, int I);
int gdmcf_cat_grad_f32(const float* dxin, int64_t lddx, const float* xt, int64_t ldxt, const float* xU, int64_t ldu, int drop_mode,
                       const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, int B, int I, void* ws,
                       size_t ws_bytes, float* grad_w, float* grad_b, void* stream);
/* The cat layer fed from device CSR rows: row b of the batch is row rows[b] of a {0,1} CSR matrix (indptr int64, indices int32).
 * gdmcf_cat_prep_input_csr_f32 is ONE launch for gdmcf_densify_rows_f32, gdmcf_onehot_noise_f32(offset = offset_noise) and
 * gdmcf_cat_prep_input_f32(offset = offset_prep): for equal inputs, seed and offsets it leaves the same bits over the whole
 * [B, ldxin] extent of xin, in xt_out[:, 0:I] and in temb_out; neither the dense rows nor the [B, 2I] image exist.  The classes
 * are `sampled` (uint8 [B, lds], non-zero = class 1; ts_U may be NULL) or drawn from ts_U [B] with gdmcf_onehot_noise_f32's
 * counters.  It also writes two bitmaps (both required; word c >> 5, bit c & 31 = column c, bits behind I are 0, words behind
 * ceil(I/32) are not written): x0bits_out, the rows -- the target gdmcf_linear_loss_fwd_bits_f32 reads -- and clsbits_out, the
 * classes.  Both offsets are by-value: the entry refuses to run while a graph step state is bound.                              */
int gdmcf_cat_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts_U,
                                 float discrete, const uint8_t* sampled, int64_t lds, uint64_t offset_noise, const int64_t* ts,
                                 const float* ca, const float* cb, int noise_mode, const float* noise, int64_t ldn, int drop_mode,
                                 const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset_prep,
                                 const float* cat_w, const float* cat_b, const float* emb_w, const float* emb_b, int E, int B, int I,
                                 float* xin, int64_t ldxin, float* xt_out, int64_t ldxt, float* temb_out, uint32_t* x0bits_out,
                                 int64_t ldx0bits, uint32_t* clsbits_out, int64_t ldclsbits, void* stream);
/* gdmcf_cat_grad_f32 with the one-hot pair taken from the two bitmaps of gdmcf_cat_prep_input_csr_f32 instead of xU:
 * xU[b,2i] = !x0 && !class, xU[b,2i+1] = x0 && class.  Same mapping, partials (gdmcf_cat_grad_ws_bytes) and reduction.
 * The four results equal gdmcf_cat_grad_f32's on the corresponding image bit for bit (the fused multiply-adds of the sum
 * dz * x_t are written out as the dense kernel is compiled, csrc/cat.hip: cat_grad_fused).                                     */
int gdmcf_cat_grad_bits_f32(const float* dxin, int64_t lddx, const float* xt, int64_t ldxt, const uint32_t* x0bits, int64_t ldx0bits,
                            const uint32_t* clsbits, int64_t ldclsbits, int drop_mode, const uint8_t* keep, int64_t ldkeep,
                            float drop_p, uint64_t seed, uint64_t offset, int B, int I, void* ws, size_t ws_bytes, float* grad_w,
                            float* grad_b, void* stream);

/* ---- NT-Xent term of the embedding backbones and its gradient (models/DNN.py:479-508, applied at :627-629; csrc/ntxent.hip) ----
 * z1 [B, ld1], z2 [B, ld2]: the two hidden activations, d columns each (what follows a row's d elements is never read).
 * float32 throughout, 2 <= B <= 4096 and 1 <= d <= 4096 (GDMCF_E_UNSUPPORTED otherwise).  No float atomics, every sum in one
 * fixed order: same inputs, same bits.  No host synchronisation, copy or allocation.
 *
 * gdmcf_ntxent_fwd_f32 replaces `torch.mm(z1, z2.t()) / temperature`, the softmax, `torch.eye(..).bool()`, `masked_select(~mask)`
 * (whose output size makes torch synchronise the stream), `.view(n, -1).sum(dim=1)`, `torch.diag`, the log and the mean of
 * nt_xent_loss (DNN.py:484-508), in three launches:
 *   S = z1 z2^T / temperature (v_mfma_f32_16x16x4_f32);  P = softmax of every row (row maximum subtracted, expf, divided by the
 *   row sum);  neg_i = sum_{j != i} P_ij, summed over the off-diagonal entries themselves (never 1 - P_ii);
 *   *loss_out = mean_i -log((P_ii + eps) / neg_i)                                                     (a device float)
 * and leaves P and three numbers per row in ws (gdmcf_ntxent_ws_bytes(B) bytes, 16-byte aligned) for the gradient.
 *
 * gdmcf_ntxent_bwd_f32 replaces what autograd runs behind `closs` (the masked_scatter of masked_select's backward, the softmax
 * backward, two torch.mm), in one launch, from the ws the forward entry left for the same z1, z2, B, d:
 *   dS_ij = P_ij (g_ij - c_i) / temperature,  g_ii = -1 / (B (P_ii + eps)),  g_ij = 1 / (B neg_i),  c_i = sum_k g_ik P_ik
 *   dz1 = scale[0] dS z2,  dz2 = scale[0] dS^T z1      (scale: a device float, NULL = 1; dz1, dz2 are OVERWRITTEN and must not
 *                                                       alias z1, z2 or ws)                                               */
size_t gdmcf_ntxent_ws_bytes(int B);
int gdmcf_ntxent_fwd_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int B, int d, float temperature, float eps,
                         void* ws, size_t ws_bytes, float* loss_out, void* stream);
int gdmcf_ntxent_bwd_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int B, int d, const void* ws, size_t ws_bytes,
                         const float* scale, float* dz1, int64_t lddz1, float* dz2, int64_t lddz2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDMCF_HIP_H */
