/*
 * nested_diffusion.h -- C ABI of libnd_hip.so, the MI355X (gfx950) implementation of the
 * nested-diffusion (LaDiNE) inference hot path, of the attacks on it, and of the training steps of the
 * mapping MLPs and of the ViT (the weight gradient and Adam / AdamW fused into one pass over the weight:
 * "training of the mapping MLPs" and "training of the ViT" below), and of the training step of the noise estimators (BatchNorm in
 * training mode forward and backward, gradient-norm clipping and Adam from materialised gradients: "training of the noise estimators").
 *
 * The reference (xingbpshen/nested-diffusion) has no FFI: its hot path is plain Python calling
 * torch ops.  Each entry point below therefore names the reference Python call(s) it replaces
 * (file:line relative to the reference checkout).  The host side that mirrors the reference's
 * Python API lives in nested_diffusion_amd/ and binds this library with ctypes.
 *
 * Conventions
 *  - plain C types only; every `*_dev` pointer is a DEVICE pointer owned by the caller
 *    (PyTorch-ROCm tensors in practice); the library never allocates device memory --
 *    the caller provides one workspace of nd_workspace_bytes().
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - every function returns 0 on success, <0 on error; nd_last_error() gives the message.
 *    No C++ exception crosses the ABI.
 *  - fp32 at the ABI: every tensor handed in or out is fp32 row-major (int64 votes aside) unless a declaration says "image".
 *    INSIDE, operands live in MFMA lane order: frag16 (fp32, the weight-streaming layers), frag32b3 (three exact bf16 pieces per
 *    fp32 value: every MFMA-bound layer -- the ViT Linear layers and attention, the ConditionalLinear blocks above 128 rows -- runs on
 *    the bf16 matrix pipe with EXACT fp32 products and fp32 accumulation; csrc/nd_b9.hpp), frag32h (fp16, the fp16-operand mode).
 *    The arithmetic is the reference's fp32 arithmetic in another summation order in every default mode.
 *  - one handle per GPU per process; not thread-safe for concurrent calls on one handle.
 */
#ifndef NESTED_DIFFUSION_H
#define NESTED_DIFFUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ND_OK 0
#define ND_ERR_ARG (-1)
#define ND_ERR_HIP (-2)
#define ND_ERR_STATE (-3)

/* activation codes for the generic linear entry points */
#define ND_ACT_NONE 0
#define ND_ACT_SOFTPLUS 1 /* torch softplus beta=1 threshold=20 (latent_model.py:130,133,176,180,183) */
#define ND_ACT_RELU 2     /* mapping/models/mlp.py:25-27 */
#define ND_ACT_GELU 3     /* exact erf GELU, timm 0.4.12 Mlp */

typedef struct nd_handle_s *nd_handle;

/* Dimensions of one ensemble: K ConditionalModel members (latent_model.py:108-167, arch 'linear',
 * guidance=True) that share shapes.  Config dims: y_dim 2, data_dim 150528, hidden 4096,
 * feature 4096 (configs/chest_x_ray.yml:5,11,14-15). */
typedef struct {
    int32_t y_dim;       /* C  = config.data.num_classes (1..8: a library limit the reference does not have -- the step head keeps a
                          *     row's C state values and C eps sums in registers; the shipped configs use 2) */
    int32_t data_dim;    /* D  = config.model.data_dim          (multiple of 16) */
    int32_t hidden_dim;  /* H  = config.model.hidden_dim        (multiple of 16) */
    int32_t feature_dim; /* F  = config.model.feature_dim       (multiple of 16) */
    int32_t n_steps;     /* T  = config.diffusion.timesteps; embed tables hold T+1 rows */
    int32_t n_members;   /* K  (1..255) */
    int32_t max_batch;   /* largest B (images) per call */
    int32_t max_rows;    /* largest M = B * mc_trials per call */
    int32_t operand_dtype; /* ND_DTYPE_F32 (0): the reference's arithmetic.  ND_DTYPE_F16 (1): weights of the five large Linear
                            * layers and their input activations are held in fp16 (products exact, fp32 accumulation, fp32
                            * epilogues, tables and state) -- BASELINE config 5; the reference has no such mode.  Needs
                            * data_dim, hidden_dim, feature_dim % 32 == 0. */
} nd_config;
#define ND_DTYPE_F32 0
#define ND_DTYPE_F16 1
/* nd_cond_config only: fp32 arithmetic as ND_DTYPE_F32 -- exact products, fp32 sums -- with the ViT's Linear layers on the bf16 matrix
 * pipe (nd_gemm_split): their weights are handed over as frag32b3 images (nd_split_rows of the fp32 [out,in] weight, made once at
 * load), embed_dim, mlp_hidden and in_chans*patch^2 must be multiples of 32.  The mapping MLPs and the attention run as in F32. */
#define ND_DTYPE_F32_SPLIT 2

/* Device pointers to ONE member's raw parameters, exactly the tensors of
 * ConditionalModel.state_dict() (key in the comment; shapes for config dims). */
typedef struct {
    const float *enc0_w, *enc0_b;                       /* encoder_x.0.{weight [H,D], bias [H]} */
    const float *bn0_w, *bn0_b, *bn0_mean, *bn0_var;    /* encoder_x.1.* [H] */
    const float *enc3_w, *enc3_b;                       /* encoder_x.3.{weight [H,H], bias} */
    const float *bn1_w, *bn1_b, *bn1_mean, *bn1_var;    /* encoder_x.4.* [H] */
    const float *enc6_w, *enc6_b;                       /* encoder_x.6.{weight [F,H], bias} */
    const float *norm_w, *norm_b, *norm_mean, *norm_var;/* norm.* [F] */
    const float *lin1_w, *lin1_b, *emb1;                /* lin1.lin.{weight [F,2C], bias}, lin1.embed.weight [T+1,F] */
    const float *un1_w, *un1_b, *un1_mean, *un1_var;    /* unetnorm1.* */
    const float *lin2_w, *lin2_b, *emb2;                /* lin2.lin.{weight [F,F], bias}, lin2.embed.weight */
    const float *un2_w, *un2_b, *un2_mean, *un2_var;    /* unetnorm2.* */
    const float *lin3_w, *lin3_b, *emb3;                /* lin3.* */
    const float *un3_w, *un3_b, *un3_mean, *un3_var;    /* unetnorm3.* */
    const float *lin4_w, *lin4_b;                       /* lin4.{weight [C,F], bias [C]} */
} nd_member_weights;

const char *nd_last_error(void);
/* "gfx950 f32 <build id>" -- lets the host assert the native library is the one loaded. */
const char *nd_version(void);

/* ---- ensemble handle --------------------------------------------------------------------- */
int nd_create(const nd_config *cfg, nd_handle *out);
int nd_destroy(nd_handle h);
/* Bytes of device workspace the handle needs (folded tables, activations, split-K slabs). */
size_t nd_workspace_bytes(const nd_config *cfg);
int nd_bind_workspace(nd_handle h, void *workspace_dev, size_t bytes);

/* Replaces ConditionalModel(...).load_state_dict(state['noise_estimator']) + .eval() + .to(device)
 * (classification_train_separately.py:685-697, 773).  Repacks the five weight matrices into the
 * workspace in fragment order (the caller may free its tensors when the call returns) and folds eval-mode BatchNorm1d, the Linear bias and the per-timestep
 * Embedding gain into scale/shift tables:  BN(g_t * (W h + b)) = a_t * (W h) + c_t. */
int nd_load_member(nd_handle h, int member, const nd_member_weights *w, void *stream);

/* alphas / one_minus_alphas_bar_sqrt, as handed to p_sample_loop (diffusion_utils.py:133;
 * built at classification_train_separately.py:215-226).  Device arrays of length T, copied. */
int nd_set_schedule(nd_handle h, const float *alphas_dev, const float *omabs_dev, int T, void *stream);

/* xe = norm(encoder_x(x)) for members [member0, member0+n_members)  -- latent_model.py:170-171.
 * t-invariant, so evaluated ONCE per (member, batch) instead of once per denoising step.
 * x_dev [B, D] row-major (images_224_flat, classification_train_separately.py:747). */
int nd_encode(nd_handle h, int member0, int n_members, const float *x_dev, int B, void *stream);

/* One eps_theta evaluation of the t-dependent trunk on the cached xe:
 * ConditionalModel.forward lines latent_model.py:172-184.  y_dev [M,C], yhat_dev [B,C],
 * eps_out_dev [M,C]; row m uses image m % B.  Used for unit parity tests and the nn.Module mirror. */
int nd_eps_theta(nd_handle h, int member, const float *y_dev, const float *yhat_dev, int t,
                 float *eps_out_dev, int B, int mc, void *stream);

/* One reverse step for one member: p_sample (diffusion_utils.py:54-92) when t >= 1 with the draw
 * z_dev [M,C] supplied, p_sample_t_1to0 (:96-111) when t == 0 (z_dev ignored, may be NULL).
 * y_dev [M,C] -> y_out_dev [M,C]; yhat_dev / ymean_dev [B,C]. */
int nd_p_sample(nd_handle h, int member, const float *y_dev, const float *yhat_dev, const float *ymean_dev,
                const float *z_dev, int t, float *y_out_dev, int B, int mc, void *stream);

/* p_sample_loop(..., only_last_sample=True) for members [member0, member0+n_members) and mc
 * Monte-Carlo trials at once (diffusion_utils.py:133-163 driven by the member x trial loop at
 * classification_train_separately.py:767-777).  M = B*mc rows per member, row m = trial*B + image.
 *   yhat_dev  [n_members, B, C]   eps_theta condition (y_0_hat)
 *   ymean_dev [n_members, B, C]   prior mean y_T_mean (same tensor in the reference, quirk Q2)
 *   noise_dev [n_members, T, M, C] the reference's RNG draws in draw order: index 0 = initial
 *              randn_like (:139), index i>=1 = the draw of p_sample at t = T-i (:67); NULL = draw them in the library
 *              (Philox, see nd_seed): throughput mode
 *   y0_out_dev [n_members, M, C]
 *   seq_out_dev optional [n_members, T+1, M, C]: y_T, y_{T-1}, ..., y_0 (only_last_sample=False)
 * The 3T+1 kernels are replayed from one hipGraph per (member range, B, mc, T, pointers) when
 * use_graph != 0.  nd_encode must have run for these members with the same B. */
int nd_sample(nd_handle h, int member0, int n_members, const float *yhat_dev, const float *ymean_dev,
              const float *noise_dev, float *y0_out_dev, float *seq_out_dev, int B, int mc, int T,
              int use_graph, void *stream);

/* SAMPLER PLAN: fewer reverse steps from the schedule a member was trained on (not a reference mode: the reference declares --skip_type,
 * --eta and --sample_type and never reads them).  With u = y - y_T_mean the forward process is plain DDPM in u, so any increasing
 * subsequence 0 <= tau_0 < .. < tau_{S-1} <= n_steps - 1 is itself a chain.  With abar_t = 1 - one_minus_alphas_bar_sqrt[t]^2, the step
 * from t = tau_j to r = tau_{j-1} (j >= 1) with eps = eps_theta(x, y, tau_j, yhat) and a draw z is
 *     sigma = eta sqrt((1 - abar_r) / (1 - abar_t)) sqrt(1 - abar_t / abar_r)                    0 <= eta <= 1
 *     cy = sqrt(abar_r / abar_t), cm = 1 - cy, ce = sqrt(1 - abar_r - sigma^2) - cy sqrt(1 - abar_t), cz = sigma
 *     y_r = fmaf(cz, z, fmaf(ce, eps, fmaf(cm, y_T_mean, cy * y)))                              (fp32, no contraction)
 * and the last one (row 0: p_sample_t_1to0 at tau_0) has cy = 1 / sqrt(abar), cm = -(1 - sqrt(abar)) / sqrt(abar), ce = -sqrt(1 - abar) /
 * sqrt(abar), cz = 0.  The caller forms the S x 4 coefficients in double and rounds once (diffusion_utils.sampler_plan).
 *   nd_set_sampler    timesteps_host [S] and coef_host [S][4] = (cy, cm, ce, cz) are HOST arrays, free again when the call returns.
 *                     The handle keeps tau on the host (baked into kernel arguments) and the coefficients in a device buffer of its own:
 *                     nd_workspace_bytes does not change.  S = 0 clears the plan (the pointers are not read).  Drops the recorded graphs.
 *                     Refused (ND_ERR_ARG) before anything is allocated or copied: "handle is NULL", "S=.. outside [0,n_steps]",
 *                     "timesteps_host / coef_host is NULL", "timesteps[j]=.. outside [0,n_steps)", "timesteps must be strictly
 *                     increasing", "coefficient [j][q] is not finite".
 *   nd_sampler_steps  S of the plan that is set, 0 for none.
 * While a plan is set nd_sample and nd_predict_batch run its S steps: they take T == S and refuse any other T without writing anything
 * (ND_ERR_STATE, "sampler plan holds S=.. steps, the call asks T=.. (nd_set_sampler)"); noise stays [n_members, T, M, C] (index 0 the
 * initial draw, index i the draw of step i), seq_out [n_members, T+1, M, C], and the library's own noise is keyed on the call's shape as
 * before.  Step i evaluates eps at embedding row tau_{S-1-i}; its head applies coefficient row S-i, the final kernel row 0.  The
 * per-step loop form runs (the one-launch form knows consecutive timesteps only; nd_loop_form returns 0).  nd_eps_theta and nd_p_sample
 * do not look at the plan.  The kernels of a plan are instantiations of their own: a handle without one launches what it always did. */
int nd_set_sampler(nd_handle h, const int32_t *timesteps_host, const float *coef_host, int S, void *stream);
int nd_sampler_steps(nd_handle h);

/* Kernel-duration probes for the roofline report: when enabled, up to 8 PAIRS of consecutive denoising steps (i, i+1) of every
 * nd_sample / nd_predict_batch graph (or eager loop) get hipEvent record nodes on the launch stream: before the head of step i, after
 * it, after the two ConditionalLinear launches of step i, and after those of step i+1.  nd_profile_read (after the stream is
 * synchronised) returns mean intervals in microseconds over the last call's probed pairs: out_us[0] head(i) + o, [1] the lin2 and
 * lin3(+lin4) launches of step i TOGETHER + o, [2] the whole unrecorded step i+1 (head + both launches) + o, [3] o = what a record
 * node adds to a loaded interval = out_us[0] - (out_us[2] - out_us[1]) -- the overheads cancel in [2] - [1], which is the head alone.
 * Mean step-block launch = (out_us[1] - out_us[3]) / 2.  *n_samples = probed pairs = min(8, (T - 1) / 2).  out_us holds 4 floats. */
int nd_set_profiling(nd_handle h, int enable);
/* Weight bytes of one step launch (block 0: lin2 of all loaded members, 1: lin3) that are read with default-policy loads and so
 * stay resident in the 256 MiB Infinity Cache from step to step; the rest is streamed from HBM with nontemporal loads.  Lets the
 * roofline report separate bytes DELIVERED to the CUs from bytes that come out of DRAM.  -1 on a bad argument. */
long long nd_resident_weight_bytes(nd_handle h, int block);
int nd_profile_read(nd_handle h, float *out_us, int *n_samples);
/* Number of hipGraph event-record nodes in the most recently BUILT nd_sample / nd_predict_batch graph (4 per probed step when
 * profiling is on, 0 when it is off; -1 if the graph could not be walked): what a test checks to know that nd_profile_read's
 * intervals are stamped on every replay and are not left over from the eager first call. */
int nd_profile_probe_nodes(nd_handle h);

/* Refilling the input buffer early.  flag: a 32-bit word in host memory the DEVICE can write (pinned / mapped host memory), or NULL to
 * switch the signal off.  With a flag set, every nd_predict_batch call or graph replay stores 1, 2, 3, ... to it (the count of calls since
 * this function was called) as soon as the last kernel that reads images_dev has run -- the im2col of the conditioner and the pack of the
 * encoder hoist, about a quarter into the batch -- so a loader may write the NEXT batch into images_dev (classification_train_separately.py:
 * 722, the .to(device) of the batch loop) while this batch's sampler is still running.  Synchronises the device; drops the recorded batch
 * graphs. */
int nd_set_input_flag(nd_handle h, uint32_t *flag_host_visible);

/* FORM OF THE SAMPLING LOOP (diffusion_utils.py:145-157, the T iterations of p_sample_loop).  mode 0: 3T+1 kernel nodes of a
 * hipGraph (head, lin2 block, lin3 + lin4 block per step).  mode 1: ONE kernel launch for the whole loop where the shape allows
 * (csrc/nd_persist.hip: 17..32 rows per member, fp32 operands, <= 8 members whose weights exceed the Infinity Cache; any other call
 * keeps mode 0): each member's workgroups stay on their CUs for all T steps and meet at per-member barriers, members `skew_us`
 * microseconds apart, so one member's reductions run under the others' weight streams.  Same bits as mode 0.  The one-launch form
 * needs every workgroup of its grid resident at once, i.e. the device to itself while it runs (one process per GPU; processes that
 * share a device select mode 0).  A handle starts in the mode ND_PERSIST names (default: see nd_create); skew_us < 0 keeps the
 * current skew.  Drops the recorded graphs.
 *   nd_loop_form      1 if the most recently recorded or enqueued loop took the one-launch form, else 0
 *   nd_persist_status synchronises the device and returns 0 when no barrier wait of a one-launch loop has been abandoned since the
 *                     last reset (1 otherwise: results of that call are invalid -- every spin is bounded, a wait of more than one
 *                     second means the grid was not resident); reset != 0 clears the flag. */
int nd_set_loop_form(nd_handle h, int mode, float skew_us);
int nd_loop_form(nd_handle h);
int nd_persist_status(nd_handle h, int reset);

/* Copy of an internal per-member activation (tests / debugging), converted from the packed layout to
 * row-major: which = 0 xe [rows<=B, F], 1 h1 [rows<=M, F], 2 h2 [rows<=M, F] -> dst_dev [rows, F];
 * which = 3 e0, 4 e1 (the encoder's two hidden activations of the last nd_encode) [rows<=B, hidden_dim] -> dst_dev [rows, hidden_dim].
 * Arguments are checked before the handle's state: ND_ERR_ARG for an unknown `which` or too many rows, also on an unbound handle. */
int nd_member_buffer(nd_handle h, int member, int which, float *dst_dev, int rows, void *stream);

/* ---- standalone operators (mapping network + unit tests) ---------------------------------- */
/* "frag16" packing of a K-contiguous matrix [R, K] (K % 16 == 0) into the MFMA fragment order the
 * weight-streaming kernels read with fully coalesced 1 KiB wave loads (layout: DESIGN.md).  Rows are
 * padded to a multiple of 16 with zeros.  Weights are packed once (mapping-MLP load time).
 * dtype ND_DTYPE_F16: the "frag32h" image (fp16, round to nearest even, K % 32 == 0) for the fp16-operand mode. */
size_t nd_packed_bytes(int R, int K, int dtype);
int nd_pack_rows(const float *src_dev, void *dst_packed_dev, int R, int K, int dtype, void *stream);

/* out[M,N] = act(scale[n] * (x[M,K] . W[N,K]^T) + shift[n]); scale/shift may be NULL (1 / 0).
 * nn.Linear + bias (+ReLU) of mapping/models/mlp.py:25-28 with shift = bias.  x and out are row-major fp32,
 * w_packed_dev is the nd_pack_rows image (same dtype) of the [N, K] nn.Linear weight.  Skinny-M weight streaming;
 * split-K across workgroups when K is large.  workspace_dev: >= nd_linear_workspace_bytes(M, K, N, dtype).
 * dtype ND_DTYPE_F16: x is rounded to fp16 on the way in, products exact, fp32 accumulation and epilogue. */
size_t nd_linear_workspace_bytes(int M, int K, int N, int dtype);
int nd_linear(const float *x_dev, const void *w_packed_dev, const float *scale_dev, const float *shift_dev,
              float *out_dev, int M, int K, int N, int act, int dtype, void *workspace_dev, size_t workspace_bytes,
              void *stream);

/* Launch plan the weight-streaming kernel would use for a Linear of this shape (host-side, no GPU work; tests / tuning):
 * out6 = {grid.x, grid.y, grid.z (k-slabs), fragment slots per workgroup, k-chunks per slab, threads per workgroup}.
 * mode 0 fused activation, 1 lin3+lin4 projection, 2 split-K partial sums. */
int nd_skinny_plan(int K, int N, int M, int n_members, int dtype, int mode, int *out6);
/* Row fragments (16 rows each) a weight-streaming workgroup keeps per pass at M rows -- the kernel's MT template argument (1, 2, 4, or
 * 5 where five save a whole pass over the weights: 65..80 rows, the reference's batch_size 70, configs/chest_x_ray.yml:66). < 0: error. */
int nd_skinny_row_fragments(int M);

/* Which kernel one ConditionalLinear block of the sampler (latent_model.py:178-184; K = N = feature_dim) runs at
 * M = B * mc_trials rows (mc_trials = 20 at classification_train_separately.py:770-771, batch_size 70 in
 * configs/chest_x_ray.yml:66 -> M = 1400), host only.  out8 = {0 weight-streaming k_skinny | 1 LDS-tiled k_cond_gemm
 * (M > 128 rows, fp32 operands), workgroups of the tiled launch, whole tiles, remainder tiles, k-split of the remainder,
 * partial sums per (row, class) handed to the step head, 128-row tiles over M, over N}. */
int nd_step_plan(int feature_dim, int M, int n_members, int dtype, int *out8);

/* Large-M GEMM for the ViT blocks: out[M,N] = act(x[M,K] . W[N,K]^T + bias[n]) (+ residual[M,N]).
 * timm 0.4.12 Attention.qkv / proj, Mlp.fc1 (GELU) / fc2, PatchEmbed.proj as GEMM
 * (call sites classification_train_separately.py:337-340).
 * workspace_dev (>= nd_gemm_workspace_bytes(M, K, N), 16-byte aligned; may be NULL/0): lets the last, partly filled round
 * of output tiles be cut along K across the idle CUs; without it every tile is computed whole (same sums, other order).
 * dtype ND_DTYPE_F32: w_dev is the fp32 [N,K] weight.  ND_DTYPE_F16 (fp16 mode; K % 32 == 0): w_dev is an fp16 [N,K] copy of it
 * (row-major, made once by the caller), x is rounded to fp16 on the fly, products exact, fp32 accumulation / epilogue / out. */
size_t nd_gemm_workspace_bytes(int M, int K, int N, int dtype);
int nd_gemm_bias_act(const float *x_dev, const void *w_dev, const float *bias_dev, const float *residual_dev,
                     float *out_dev, int M, int K, int N, int act, int dtype, void *workspace_dev, size_t workspace_bytes,
                     void *stream);

/* The same Linear layers (timm 0.4.12 Attention.qkv / proj, Mlp.fc1 / fc2, PatchEmbed.proj; call sites
 * classification_train_separately.py:337-346) on the bf16 matrix pipe WITH EXACT fp32 PRODUCTS: every fp32 operand value is held as
 * its three exact bf16 pieces a = a1 + a2 + a3 (8 + 8 + 8 significand bits), the nine piece products of a pair are exact in fp32 and
 * are accumulated in fp32 by v_mfma_f32_16x16x32_bf16 -- the reference's arithmetic (exact products, fp32 sums) in another summation
 * order, at 9/16 of the matrix-pipe cycles of the f32-input MFMA.  Operands are "frag32b3" images (csrc/nd_b9.hpp): made ONCE by
 * nd_split_rows (weights at load) or written directly by the producing operator (nd_layernorm_split, nd_gemm_split's out_split, ...).
 *   nd_split_bytes(rows, K)   bytes of the image of a [rows, K] matrix (rows padded to 16; K % 32 == 0), 0 on a bad shape
 *   nd_split_rows             x [rows, K] fp32 row-major -> image;   nd_join_rows: the inverse (exact), for tests
 *   nd_gemm_split             out[M,N] = act(x . w^T + bias) (+ residual): x_split_dev image of [M,K], w_split_dev image of [N,K];
 *                             out_dev fp32 [M,N] and / or out_split_dev = image of the result (N % 32 == 0) for the next layer; one of the
 *                             two may be NULL.  workspace as nd_gemm_bias_act (>= nd_gemm_split_workspace_bytes, may be NULL). */
size_t nd_split_bytes(int rows, int K);
int nd_split_rows(const float *x_dev, void *out_split_dev, int rows, int K, void *stream);
int nd_join_rows(const void *in_split_dev, float *x_dev, int rows, int K, void *stream);
size_t nd_gemm_split_workspace_bytes(int M, int K, int N);
int nd_gemm_split(const void *x_split_dev, const void *w_split_dev, const float *bias_dev, const float *residual_dev, float *out_dev,
                  void *out_split_dev, int M, int K, int N, int act, void *workspace_dev, size_t workspace_bytes, void *stream);

/* nn.LayerNorm(eps) over the last dim: x [rows, dim] -> out.  timm Block.norm1/norm2 (eps 1e-6).
 * nd_layernorm_split: the same values written as the frag32b3 image of [rows, dim] (dim % 32 == 0; nd_split_bytes(rows, dim) bytes):
 * the input of the nd_gemm_split that follows each LayerNorm of a ViT block. */
int nd_layernorm(const float *x_dev, const float *gamma_dev, const float *beta_dev, float *out_dev,
                 int rows, int dim, float eps, void *stream);
int nd_layernorm_split(const float *x_dev, const float *gamma_dev, const float *beta_dev, void *out_split_dev,
                       int rows, int dim, float eps, void *stream);

/* timm 0.4.12 Attention core: qkv [B, N, 3, heads, d] (the qkv Linear's output, unpermuted) ->
 * out [B, N, heads*d] = softmax(q k^T * d^-0.5) v, heads concatenated.  d must be 64.
 * dtype ND_DTYPE_F16 (fp16 mode): q, k, v and the normalised probabilities rounded to fp16, f16 MFMA, fp32 softmax/accumulate/out. */
int nd_attention(const float *qkv_dev, float *out_dev, int B, int N, int heads, int d, int dtype, void *stream);
/* The fp32 attention with its result written as the frag32b3 image of [B*N, heads*d] (the input of the proj nd_gemm_split). */
int nd_attention_split(const float *qkv_dev, void *out_split_dev, int B, int N, int heads, int d, void *stream);

/* The same attention with BOTH contractions on the bf16 matrix pipe, exact fp32 products (timm 0.4.12 Attention.forward; call sites
 * classification_train_separately.py:339-340).  Its operands are "qkv images": per (image, head) the q and k rows as frag32b3 blocks and
 * v transposed (layout: B9AttLayout, csrc/nd_b9.hpp), written directly by the qkv Linear's epilogue:
 *   nd_qkv_images_supported  1 where the form applies: N % 4 == 0, N <= 256, heads * 64 a multiple of 128
 *   nd_qkv_images_bytes      size of the image buffer for B images of N tokens
 *   nd_gemm_split_qkv        qkv Linear: x_split_dev image of [B*N, K], w_split_dev image of the [3*heads*64, K] weight, bias [3*heads*64]
 *   nd_attention_images      softmax(q k^T / 8) v from the images; out_dev fp32 [B*N, heads*64] or (out_is_split) its frag32b3 image */
int nd_qkv_images_supported(int N, int heads);
size_t nd_qkv_images_bytes(int B, int N, int heads);
int nd_gemm_split_qkv(const void *x_split_dev, const void *w_split_dev, const float *bias_dev, void *qkv_images_dev, int B, int N, int heads,
                      int K, void *stream);
int nd_attention_images(const void *qkv_images_dev, void *out_dev, int out_is_split, int B, int N, int heads, void *stream);

/* PatchEmbed im2col: img [B, Cin, Himg, Wimg] NCHW -> cols [B * (Himg/p) * (Wimg/p), Cin*p*p] so that
 * Conv2d(k=p, s=p) becomes nd_gemm_bias_act with the conv weight viewed [embed, Cin*p*p]. */
int nd_patchify(const float *img_dev, float *cols_dev, int B, int Cin, int Himg, int Wimg, int p, void *stream);
/* The same im2col written as the frag32b3 image of its [B * (Himg/p) * (Wimg/p), Cin*p*p] result (Cin*p*p % 32 == 0). */
int nd_patchify_split(const float *img_dev, void *cols_split_dev, int B, int Cin, int Himg, int Wimg, int p, void *stream);

/* softmax over the last dim of [rows, C] (classification_train_separately.py:755-758). */
int nd_softmax_rows(const float *x_dev, float *out_dev, int rows, int C, void *stream);

/* Aggregation: samples [S, B, C] (S = K*mc, member-major then trial) ->
 *   prob_out [B, C]  = mean_s softmax(-(y-1)^2 / temperature)   (convert_to_prob + compute_ensemble_confidence,
 *                      classification_train_separately.py:392-398, 425-447)
 *   vote_out [B] int64 = mode_s argmax_c y  (ties -> smallest label; majority_voting_for_mc_samples :51-68)
 *   Non-finite y follow torch: argmax treats a NaN as the maximum and takes the first one; a sample whose logits hold a NaN
 *   or are all -inf (every |y| so large that (y-1)^2 overflows) has NaN probabilities, and so has the image's prob_out row.
 *   probs_out optional [S, B, C]: per-sample probabilities (what the reference leaves in mc_samples, quirk Q4) */
int nd_aggregate(const float *samples_dev, float *prob_out_dev, int64_t *vote_out_dev, float *probs_out_dev,
                 int S, int B, int C, float temperature, void *stream);

/* ---- in-library noise (throughput mode) ------------------------------------------------------------------
 * The reference draws its Gaussian noise inside the loop with the global torch generator (diffusion_utils.py:67, 139:
 * randn_like); CPU torch.randn cannot be reproduced on a device, so parity runs pass the draws in (noise_dev).  With
 * noise_dev == NULL, nd_sample / nd_predict_batch draw them here: Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit
 * seed, counter = (global image index, trial | member << 16 | class-quad << 24, draw index i (0 = y_T, i = the draw of
 * p_sample at t = T-i), batch counter); the four 32-bit outputs give four normals by Box-Muller (classes 4q..4q+3).
 * The draws of image g do not depend on how a batch is sharded over ranks (first_image = the global index of this rank's
 * first image), and the batch counter -- kept on the device, advanced by the sampler itself -- makes successive batches
 * differ.  nd_seed resets it to 0.  Synchronises the device (rare: once per run). */
int nd_seed(nd_handle h, uint64_t seed, uint32_t first_image);
/* The generator's device-resident state for a resumable run: out[0] = the seed, out[1] = batch counter | first_image << 32.
 * nd_rng_state reads it once every sampling loop enqueued so far has advanced the counter; nd_set_rng_state puts a state read
 * earlier back, so the next nd_sample / nd_predict_batch draws what it would have drawn then.  Both synchronise the device as
 * nd_seed does (rare: once per snapshot / resume); a NULL handle or pointer is ND_ERR_ARG. */
int nd_rng_state(nd_handle h, uint64_t out[2]);
int nd_set_rng_state(nd_handle h, const uint64_t in[2]);
/* The same generator as a standalone operator (tests, known-answer checks): out_dev [n_members, T, mc*B, C], row = trial*B + b. */
int nd_philox_normal(float *out_dev, int n_members, int T, int B, int mc, int C, uint64_t seed, uint32_t batch_counter,
                     uint32_t first_image, void *stream);
/* Raw Philox4x32-10 blocks (known-answer test): out_dev[4*i..4*i+3] = philox(counter = ctr_dev[4*i..], key). */
int nd_philox_raw(const uint32_t *ctr_dev, uint32_t *out_dev, int n, uint32_t key0, uint32_t key1, void *stream);

/* ---- conditioner: the mapping network (classification_train_separately.py:249-275, 330-348) -------------------
 * cond_pred_model = {'vit': timm 0.4.12 vit_base_patch16_224, 'mlps': [mapping/models/mlp.py::Classifier] * K}.
 * The handle holds POINTERS to the caller's device tensors (the caller keeps them alive, as a torch module does) and one
 * caller-provided workspace for the activations. */
typedef struct nd_cond_s *nd_cond;
typedef struct {
    int32_t img_size, patch, in_chans;   /* 224, 16, 3 */
    int32_t embed_dim, num_heads;        /* 768, 12 (head dim must be 64) */
    int32_t mlp_hidden;                  /* 3072 (timm Mlp hidden = 4 * embed) */
    int32_t n_blocks;                    /* ViT blocks available to nd_vit_block (>= n_mlps) */
    int32_t n_mlps;                      /* K mapping MLPs: MLP i reads the tokens after blocks[0..i] (:336-345) */
    int32_t mlp_widths[3];               /* 4096, 2048, 128 (mapping/models/mlp.py:12-18) */
    int32_t num_classes;                 /* C */
    int32_t max_batch;
    int32_t max_tokens;                  /* tokens per image nd_vit_block may be called with (196 on the mapping path, 197 with
                                          * the cls token of the full forward) */
    int32_t operand_dtype;               /* ND_DTYPE_F32 | ND_DTYPE_F16 (Linear weights fp16 row-major, MLP weights frag32h) */
    float ln_eps;                        /* 1e-6: timm's norm_layer = partial(nn.LayerNorm, eps=1e-6) */
} nd_cond_config;
/* timm PatchEmbed.proj viewed [embed, in_chans*patch*patch] (+ bias); fp32, or fp16 in the fp16 mode. */
typedef struct { const void *proj_w; const float *proj_b; } nd_patch_embed_weights;
/* One timm Block: norm1, attn.qkv [3E,E], attn.proj [E,E], norm2, mlp.fc1 [4E,E], mlp.fc2 [E,4E]; Linear weights row-major
 * [out,in] (nn.Linear layout) in fp32 (ND_DTYPE_F32) or fp16 (ND_DTYPE_F16), or frag32b3 images of them (ND_DTYPE_F32_SPLIT: nd_split_rows;
 * the same holds for nd_patch_embed_weights.proj_w viewed [embed, in_chans*patch^2]); everything else fp32. */
typedef struct {
    const float *norm1_w, *norm1_b;
    const void *qkv_w;  const float *qkv_b;
    const void *proj_w; const float *proj_b;
    const float *norm2_w, *norm2_b;
    const void *fc1_w;  const float *fc1_b;
    const void *fc2_w;  const float *fc2_b;
} nd_vit_block_weights;
/* One mapping MLP: linear1..4 weights as nd_pack_rows images (same dtype as the config) + fp32 biases. */
typedef struct { const void *w_packed[4]; const float *bias[4]; } nd_mlp_weights;

size_t nd_cond_workspace_bytes(const nd_cond_config *cfg);
int nd_cond_create(const nd_cond_config *cfg, nd_cond *out);
int nd_cond_destroy(nd_cond c);
const nd_cond_config *nd_cond_get_config(nd_cond c);
int nd_cond_bind_workspace(nd_cond c, void *workspace_dev, size_t bytes);
int nd_cond_set_patch_embed(nd_cond c, const nd_patch_embed_weights *w);
int nd_cond_set_block(nd_cond c, int block, const nd_vit_block_weights *w);
int nd_cond_set_mlp(nd_cond c, int i, const nd_mlp_weights *w);

/* timm 0.4.12 Block.forward on tokens [B, N, embed] (pre-LN: x += attn(norm1(x)); x += mlp(norm2(x)); exact-erf GELU):
 * the calls `vit.blocks[j](tmp)` at classification_train_separately.py:339-340.  tok_out_dev may alias tok_in_dev. */
int nd_vit_block(nd_cond c, int block, const float *tok_in_dev, float *tok_out_dev, int B, int N, void *stream);

/* Diffusion.compute_guiding_prediction (:330-345) for the K mapping members: patch_embed (no cls token, no pos_embed; pos_drop
 * is the identity in eval), blocks[0..i] with the prefix SHARED between members (15 -> K block evaluations; eval-mode blocks
 * are deterministic, same values), mlps[i] right after block i.  images_dev [B, in_chans, img, img] ->
 * logits_out_dev [K, B, C]; yhat_out_dev (optional) [K, B, C] = softmax(logits, dim=1) (:755-758).
 * The never-sampled (K+1)-th element, vit(x) (:346, quirk Q1), is not computed here.  No allocation, no synchronisation:
 * capturable into a hipGraph. */
int nd_guiding_prediction(nd_cond c, const float *images_dev, float *logits_out_dev, float *yhat_out_dev, int B, void *stream);

/* ---- the whole hot path of one test batch as ONE launch (classification_train_separately.py:749-794) ----------
 * guiding prediction -> softmax -> encoder hoist of every member -> K x mc p_sample_loops -> convert_to_prob / mean / vote,
 * replayed from one hipGraph per (pointers, B, mc, T) when use_graph != 0.  Device pointers, caller-owned:
 *   images_dev [B, in_chans, img, img] (flattened [B, D] for the noise estimators, :747)
 *   noise_dev  [K, T, mc*B, C] in the reference's draw order, or NULL for in-library Philox noise (nd_seed)
 *   out->samples [K*mc, B, C] raw y_0, member-major then trial (the order of mc_samples, :767-784)
 *   out->prob [B, C], out->vote [B] int64, out->probs [K*mc, B, C] (optional), out->yhat [K, B, C]
 * K = the ensemble handle's n_members, all loaded, K <= the conditioner's n_mlps: member k is conditioned on mapping MLP k, and only
 * the first K mapping MLPs (and the prefix blocks they need) are evaluated -- the reference samples selected_block_indices ∩ the
 * available diffusion checkpoints (:275, :769), e.g. 3 noise estimators beside 5 mapping MLPs. */
typedef struct { float *samples; float *prob; int64_t *vote; float *probs; float *yhat; } nd_batch_out;
int nd_predict_batch(nd_handle h, nd_cond c, const float *images_dev, const float *noise_dev, const nd_batch_out *out,
                     int B, int mc, int T, float temperature, int use_graph, void *stream);

/* ---- reporting tail of test_atk (classification_train_separately.py:801-838) --------------------- */
/* Per-image spread of the S = K*mc per-sample probabilities (what the reference keeps in pred_mc, quirk Q4):
 *   piw_out[B,C] = quantile(q_hi) - quantile(q_lo) over the samples (torch.quantile semantics: linear
 *                  interpolation at rank q*(S-1));  compute_mean_piws_for_class :108-114 uses 0.025 / 0.975
 *   var_out[B,C] = unbiased variance over the samples (NaN at S = 1);  calculate_variances :166-172
 *   A NaN among the S values of one (b, c) gives NaN piw_out and var_out for that (b, c), as torch.quantile and var do; every
 *   other (b, c) is unaffected.
 * probs_dev [S,B,C]. */
int nd_sample_stats(const float *probs_dev, float *piw_out_dev, float *var_out_dev, int S, int B, int C,
                    float q_lo, float q_hi, void *stream);

/* The numbers test_atk prints, over the whole test set (N images):
 *   out[0]        majority-vote accuracy                                   (compute_accuracy :801-807)
 *   out[1]        ECE: n_bins-bin l1 calibration error (torchmetrics 0.11.4 MulticlassCalibrationError) of
 *                 convert_to_prob(prob_mean) -- the reference passes the averaged probabilities with prob_in=False,
 *                 so they are transformed once more (:413-423, :812); kept as written
 *   out[2+c], out[2+C+c]       mean PIW of class c over correct / incorrect votes (NaN if none; :124-140)
 *   out[2+2C+c], out[2+3C+c]   mean variance of class c over correct / incorrect votes (0 if none; :150-172)
 * piw_dev, var_dev, prob_mean_dev [N,C]; vote_dev, target_dev [N] int64; out_dev [2+4C]. */
int nd_report(const float *piw_dev, const float *var_dev, const float *prob_mean_dev, const int64_t *vote_dev,
              const int64_t *target_dev, float *out_dev, int N, int C, float temperature, int n_bins, void *stream);

/* ---- input gradient of the full ViT and the Linf attacks (the reference attacks cond_pred_model['vit'] with foolbox 3.x:
 * attack.py, classification_train_separately.py:661-667, utils.py:258-269).  All fp32; only the input gradient is formed.
 * The Linear layers' input gradients are nd_gemm_split calls with the frag32b3 image of W^T as the weight operand.
 *   nd_layernorm_bwd      LayerNorm input gradient: out = rstd * (gg - mean(gg) - xh * mean(gg * xh)) (+ residual), gg = g * gamma,
 *                         xh = (x - mean) * rstd, mean / rstd recomputed from x as nd_layernorm does; out fp32 [rows, dim] and / or
 *                         out_split its frag32b3 image (dim % 32 == 0); either may be NULL, not both.  dim % 4 == 0, dim <= 2048.
 *   nd_gelu_split         GELU (exact erf, the fc1 epilogue's expression) of u [rows, cols]: the frag32b3 image (and optionally fp32
 *                         out) -- the fc2 operand when fc1 runs without its activation so that u is kept.  cols % 32 == 0.
 *   nd_gelu_bwd_split     dg * gelu'(u) as the frag32b3 image (and optionally fp32 out).
 *   nd_attention_bwd      qkv fp32 [B*N, 3*heads*64] (timm layout), o = the forward output [B*N, heads*64], dout its gradient ->
 *                         dqkv fp32 [B*N, 3*heads*64] and / or its frag32b3 image.  P is recomputed from q, k; one workgroup per
 *                         (image, head), no atomics (bitwise reproducible).  1 <= N <= 208, d = 64.
 *   nd_xent_head_bwd      d = softmax(logits) - onehot(label) (gradient of the summed cross-entropy), dfeat [B, E] = d . head_w
 *                         ([C, E]); loss [B] (may be NULL) = logsumexp(logits) - logits[label].  C <= 1024.  d at the label is
 *                         p - 1 in fp32: 0 once 1 - p < 2^-24, as in torch's fp32 softmax.
 *   nd_unpatchify         the exact inverse permutation of nd_patchify: cols [B*(H/p)*(W/p), Cin*p*p] -> img [B, Cin, H, W].
 *   nd_linf_step          out = clip(x0 + clip(x + alpha * sign(grad) - x0, -eps, eps), lo, hi), sign(0) = 0 and a NaN
 *                         gradient is no step (sign(NaN) = 0, where torch.sign gives NaN), each operation one
 *                         rounded fp32 op in this order (foolbox: step, project, clip to the bounds).  grad NULL: no step (with
 *                         lo = -inf, hi = inf this is foolbox's final clip_perturbation).  n elements.
 *   nd_linf_random_start  out = clip(x0 + eps * w, lo, hi) for B images of per_image elements (per_image % 4 == 0).  Element 4q + e of
 *                         image b draws word e of Philox4x32-10 (nd_rng) with key = (seed low word, seed high word) and
 *                         counter = (first_image + b, q, restart, ND_LINF_START_TAG); the word x becomes
 *                         u = float(x >> 8) * 2^-24 (exact, [0, 1)), w = 2u - 1 (exact, [-1, 1)), then eps * w and x0 + that are
 *                         single fp32 roundings.  first_image = the global index of the first image (its index in the dataset or
 *                         test stream): an image draws the same start at any batch size and on any rank. */
#define ND_LINF_START_TAG 0x41544B31u
int nd_layernorm_bwd(const float *x_dev, const float *gamma_dev, const float *g_dev, const float *residual_dev, float *out_dev,
                     void *out_split_dev, int rows, int dim, float eps, void *stream);
int nd_gelu_split(const float *u_dev, float *out_dev, void *out_split_dev, int rows, int cols, void *stream);
int nd_gelu_bwd_split(const float *u_dev, const float *dg_dev, float *out_dev, void *out_split_dev, int rows, int cols, void *stream);
int nd_attention_bwd(const float *qkv_dev, const float *o_dev, const float *dout_dev, float *dqkv_dev, void *dqkv_split_dev,
                     int B, int N, int heads, void *stream);
int nd_xent_head_bwd(const float *logits_dev, const int64_t *labels_dev, const float *head_w_dev, float *dfeat_dev, float *loss_dev,
                     int B, int C, int E, void *stream);
int nd_unpatchify(const float *cols_dev, float *img_dev, int B, int Cin, int Himg, int Wimg, int p, void *stream);
int nd_linf_step(const float *x_dev, const float *x0_dev, const float *grad_dev, float *out_dev, size_t n, float alpha, float eps,
                 float lo, float hi, void *stream);
int nd_linf_random_start(const float *x0_dev, float *out_dev, int B, size_t per_image, uint64_t seed, uint32_t first_image,
                         uint32_t restart, float eps, float lo, float hi, void *stream);

/* ---- AutoAttack's APGD-CE, Linf (autopgd_base.py attack_single_run; the listing: nested_diffusion_amd/autoattack.py).  B images of
 * per_image fp32 elements (per_image % 4 == 0, 1 <= B <= 65535, images 16-byte aligned); every operation one rounded fp32 op in the
 * listing's order (contraction off), so a float32 restatement on the host reproduces every array bit for bit.  No entry point
 * allocates, copies synchronously or synchronises: an iteration (input gradient, control, update) can be captured.
 *   nd_apgd_random_start  out = clip(x0 + eps * (t / (m + 1e-12)), lo, hi).  Element 4q + e of row b draws word e of Philox4x32-10 with
 *                         key = (seed low word, seed high word) and counter = (index[b] (low word), q, restart, ND_APGD_START_TAG),
 *                         t = 2u - 1 as in nd_linf_random_start (exact); m = max |t| over the row (exact in any order).  index: int64
 *                         [B], the GLOBAL image index of each row, so a row of a compacted subset (a restart over the images not yet
 *                         fooled) draws what it draws in the full batch.  m_ws: B uint32 of workspace (zeroed here, on the stream).
 *   nd_apgd_control       per-image state of one iteration, one thread per image.  iter = -1 initialises from the start point:
 *                         acc = pred, loss_best = loss_best_last_check = loss, reduced_last_check = 1, step = step0 (2 eps),
 *                         loss_steps [n_iter, B] = 0, flags = 0.  0 <= iter < n_iter: pred = (argmax logits == label; the first maximal
 *                         index, a NaN logit never wins in any column; a row whose logits are all NaN yields index 0), acc &= pred,
 *                         loss_steps[iter] = loss, improved = loss > loss_best (then loss_best = loss); k > 0 is a checkpoint of
 *                         length k (the host passes the fixed schedule, 0 <= k <= iter+1):
 *                         cnt = #{c < k : loss_steps[iter-c] > loss_steps[iter-c-1]} (row -1 is row n_iter-1, torch's negative index),
 *                         osc = cnt <= k * rho || (!reduced_last_check && loss_best_last_check >= loss_best), reduced_last_check = osc,
 *                         loss_best_last_check = loss_best, and where osc: step /= 2 and restore.  flags [B] int32 =
 *                         ND_APGD_NOT_PRED | ND_APGD_IMPROVED | ND_APGD_RESTORE.  logits [B, C] fp32 (C <= 1024), labels int64,
 *                         loss [B]; step, loss_best, loss_best_last_check fp32 [B]; reduced_last_check, acc int32 [B].
 *   nd_apgd_update        per element of row b with flags f = flags[b] (flags NULL: none): NOT_PRED: x_best_adv = x_adv; IMPROVED:
 *                         x_best = x_adv, grad_best = grad; RESTORE: the iterate becomes x_best and its gradient grad_best (grad itself
 *                         is read-only).  do_step: then the momentum step with coefficient a (1 for the first step, 0.75 after):
 *                         g2 = xa - x_adv_old, x_adv_old = xa, z = clip(min(max(xa + step[b] * sign(g), x - eps), x + eps), 0, 1),
 *                         x_adv = clip(min(max((xa + (z - xa) * a) + g2 * (1 - a), x - eps), x + eps), 0, 1), sign(NaN) = 0 (no step).
 *                         Without the step a restored row's x_adv is written with x_best.  The first step (no flags, a = 1) expects
 *                         x_adv_old = x_adv: g2 = 0. */
#define ND_APGD_START_TAG 0x41504731u
#define ND_APGD_NOT_PRED 1
#define ND_APGD_IMPROVED 2
#define ND_APGD_RESTORE 4
int nd_apgd_random_start(const float *x0_dev, const int64_t *index_dev, float *out_dev, uint32_t *m_ws_dev, int B, size_t per_image,
                         uint64_t seed, uint32_t restart, float eps, float lo, float hi, void *stream);
int nd_apgd_control(const float *logits_dev, const int64_t *labels_dev, const float *loss_dev, float *step_dev, float *loss_best_dev,
                    float *loss_best_last_check_dev, int32_t *reduced_last_check_dev, int32_t *acc_dev, float *loss_steps_dev,
                    int32_t *flags_dev, int B, int C, int n_iter, int iter, int k, float rho, float step0, void *stream);
int nd_apgd_update(const float *x_dev, float *x_adv_dev, float *x_adv_old_dev, const float *grad_dev, float *x_best_dev,
                   float *grad_best_dev, float *x_best_adv_dev, const int32_t *flags_dev, const float *step_dev, int B, size_t per_image,
                   float eps, float a, int do_step, void *stream);

/* ---- the Square attack, Linf (autoattack's square.py, the score-based member of AutoAttack; the listing: nested_diffusion_amd/square.py).
 * B images [B, Cin, H, W] fp32, contiguous (1 <= B <= 65535, 1 <= Cin <= 32, 1 <= H, W <= 4096); a query changes one s x s window per image
 * (1 <= s <= min(H, W)).  Windows start anywhere and W need not be a multiple of 4: window accesses are scalar fp32, coalesced along w,
 * and nothing assumes 16-byte alignment inside an image.  Every value is one rounded fp32 op in the listed order (contraction off), so a
 * float32 restatement on the host reproduces every array bit for bit.  No entry point allocates, copies synchronously or synchronises:
 * a query (propose, the model's forward pass, accept, commit) can be captured.  Draws are Philox4x32-10 with key = (seed low word, seed
 * high word), keyed on index: int64 [B], the GLOBAL image index of each row (its low word), so a row of a compacted subset, of another
 * batch size or of another rank draws what it draws in the full run.  A row is ACTIVE while margin_min[b] > 0; any other value (<= 0,
 * -0.0, NaN) freezes it.
 *   nd_square_init        the vertical-stripe start over whole images: x_best[b,c,h,w] = x_new[b,c,h,w] = clip(x0 + eps * sigma(b,c,w), lo, hi).
 *                         With j = c * W + w, sigma = +1 if the top bit of word j % 4 of philox(counter = (index[b], j / 4, restart,
 *                         ND_SQUARE_INIT_TAG)) is set, else -1: it does not depend on h.
 *   nd_square_propose     per active row (a frozen row is not touched at all): p = philox(counter = (index[b], iter, restart,
 *                         ND_SQUARE_STEP_TAG)); vh = (uint64(p0) * (H - s + 1)) >> 32, vw = (uint64(p1) * (W - s + 1)) >> 32;
 *                         d_c = +2eps if bit c of p2 is set, else -2eps, 2eps = eps + eps in fp32; over the window [vh, vh + s) x [vw, vw + s)
 *                         of every channel only: x_new = clip(min(max(x_best + d_c, x0 - eps), x0 + eps), lo, hi); win[b] = (vh, vw),
 *                         int32 [B, 2].  iter >= 0.
 *   nd_square_accept      one thread per image.  margin = scores[label] - max_{j != label} scores[j], one fp32 subtraction (the first
 *                         maximal index wins ties); any NaN score in the row (or a label outside [0, C)) makes the margin NaN, and a NaN
 *                         margin is never accepted and never counts as fooled.  loss = margin.  iter = -1 initialises: margin_min = margin,
 *                         loss_min = loss, n_queries = 1, flags = 0.  iter >= 0, only where margin_min > 0 on entry: improved =
 *                         loss < loss_min (then loss_min = loss); accept = improved || margin <= 0 (then margin_min = margin);
 *                         n_queries += 1; flags[b] = ND_SQUARE_ACTIVE | (accept ? ND_SQUARE_ACCEPT : 0).  A frozen row gets flags = 0 and
 *                         nothing else changes.  scores [B, C] fp32 (2 <= C <= 1024), labels int64 [B]; margin_min, loss_min fp32 [B];
 *                         n_queries, flags int32 [B].
 *   nd_square_commit      over the window win[b] only (the s of the propose): ACTIVE and ACCEPT: x_best = x_new; ACTIVE alone: x_new = x_best,
 *                         which takes the candidate back; otherwise nothing.  A corner that does not keep the window inside the image is
 *                         ignored.  After every commit x_new == x_best on every element of every row: the model reads x_new directly and
 *                         no per-query copy of an image exists.
 * The three launches of a query are kept apart on purpose: the window a commit restores and the window the next propose writes overlap
 * in the same row, and stream order between the two launches keeps "restore, then perturb" in that order. */
#define ND_SQUARE_INIT_TAG 0x53514931u
#define ND_SQUARE_STEP_TAG 0x53515331u
#define ND_SQUARE_ACTIVE 1
#define ND_SQUARE_ACCEPT 2
int nd_square_init(const float *x0_dev, const int64_t *index_dev, float *x_best_dev, float *x_new_dev, int B, int Cin, int H, int W,
                   uint64_t seed, uint32_t restart, float eps, float lo, float hi, void *stream);
int nd_square_propose(const float *x0_dev, const float *x_best_dev, float *x_new_dev, const int64_t *index_dev, const float *margin_min_dev,
                      int32_t *win_dev, int B, int Cin, int H, int W, int s, int iter, uint64_t seed, uint32_t restart, float eps, float lo,
                      float hi, void *stream);
int nd_square_accept(const float *scores_dev, const int64_t *labels_dev, float *margin_min_dev, float *loss_min_dev, int32_t *n_queries_dev,
                     int32_t *flags_dev, int B, int C, int iter, void *stream);
int nd_square_commit(float *x_best_dev, float *x_new_dev, const int32_t *win_dev, const int32_t *flags_dev, int B, int Cin, int H, int W, int s,
                     void *stream);

/* ---- the Square attack, L2 (the L2 branch of autoattack's square.py; the listing: nested_diffusion_amd/square.py); csrc/nd_square_l2.hip.
 * B images [B, Cin, H, W] fp32, contiguous (1 <= B <= 65535, 1 <= Cin <= 32, 5 <= H, W <= 4096).  Unlike the Linf form a query rewrites the
 * whole perturbation: it moves norm budget from window w2 to window w1 (both of odd side s, 3 <= s <= min(H, W)) and renormalises the image
 * to the eps-sphere, so it needs per-image sums over masked regions and a whole-image write.  Every elementwise value is one rounded fp32
 * op in the listed order (contraction off); given the sums a call reports, a float32 restatement on the host reproduces every array bit
 * for bit.  Sums are fp32, without floating-point atomics, in an order fixed by (Cin, H, W, s, the windows): a wave owns one row (c, h) at
 * a time, a lane the quads w = 4k .. 4k + 3 of it with k = lane, lane + 64, ..., their terms added in ascending w; a workgroup folds its
 * 256 threads and writes one partial, and the next launch folds the <= ND_L2_MAX_PARTS partials of the image with the same tree.  Neither B,
 * the row's position in the batch nor the alignment of the arrays changes a bit: where W % 4 == 0 and the arrays are 16-byte aligned a
 * quad is one 16-byte access, otherwise four scalar ones (W = 30, 5 x 5 images and odd addresses work), with the same terms in the same
 * order.  Every argument error (ND_ERR_ARG) is found before any HIP call.  No entry point allocates, copies synchronously or
 * synchronises; one entry point enqueues several kernels on `stream`, and a query stays capturable.  Draws are Philox4x32-10 with key =
 * (seed low word, seed high word), keyed on index: int64 [B], the GLOBAL image index of each row (its low word).  A row is ACTIVE while
 * margin_min[b] > 0; any other value (<= 0, -0.0, NaN) freezes it.  ws: B * nd_square_l2_ws_floats(Cin, H, W) floats (the partials;
 * written before they are read).  eta(s): float [s, s], the unit-norm pattern of the listing, built by the host in float64 and rounded
 * once; eta_t is eta or, where the transpose bit is set, its transpose.
 *   nd_square_l2_ws_floats  floats of workspace per image (0 where Cin, H or W is out of range).
 *   nd_square_l2_init       s0 = min(H, W) / 5, nh = H / s0, nw = W / s0, oh = (H - nh * s0) / 2, ow = (W - nw * s0) / 2.  Tile t = th * nw + tw
 *                           covers rows oh + th * s0 .. and columns ow + tw * s0 ..; q = philox(counter = (index[b], t, restart,
 *                           ND_SQUARE_L2_INIT_TAG)); sigma_c = +1 if bit c of q0 is set, else -1; the tile holds eta(s0) transposed if the
 *                           top bit of q1 is set.  D0 = sigma_c * eta_t(s0) on the tiles, 0 on the margins; sums[b] = sum D0^2;
 *                           x_best = x_new = clip(x0 + D0 / (1e-12 + sqrt(sums[b])) * eps, lo, hi).  Two launches.
 *   nd_square_l2_propose    per active row (a frozen row is not touched at all: neither its image, its win nor its sums), with
 *                           D = x_best - x0: p = philox(counter = (index[b], iter, restart, ND_SQUARE_L2_STEP_TAG)); vh1 = (uint64(p0) *
 *                           (H - s + 1)) >> 32, vw1 = (uint64(p1) * (W - s + 1)) >> 32, vh2 and vw2 likewise from p2 and p3;
 *                           q = philox(counter = (index[b], iter, restart, ND_SQUARE_L2_SIGN_TAG)); sigma_c = +1 if bit c of q0 is set,
 *                           else -1; transpose = the top bit of q1.  win[b] = (vh1, vw1, vh2, vw2), int32 [B, 4].  Then
 *                               S_w1 = sum_{w1} D^2, S_all = sum D^2, S_mask = sum_{w1 u w2} D^2, S_out = sum_{outside w1 u w2} D^2
 *                               u = sigma_c * eta_t(s)[dh, dw] + D[w1] / (1e-12 + sqrt(S_w1));  S_u = sum_{w1} u^2
 *                               scale = sqrt(max(eps * eps - sqrt(S_all) * sqrt(S_all), 0) / Cin + sqrt(S_mask) * sqrt(S_mask))
 *                               D' = D;  D'[w2] = 0;  D'[w1] = u / (1e-12 + sqrt(S_u)) * scale   (w1 wins where the windows overlap)
 *                               S_new = sum_{w1} D'^2;  x_new = clip(x0 + D' / (1e-12 + sqrt(S_out + S_new)) * eps, lo, hi)
 *                           over the whole image.  sums [ND_SQUARE_L2_SUMS, B] receives (S_w1, S_all, S_mask, S_out, S_u, S_new) at rows
 *                           ND_SQUARE_L2_S_*: exactly the values the elementwise passes used.  Four launches: the masked sums, the two
 *                           window passes, the write; u and D' are recomputed where they are needed (the same bits), never stored.
 *                           x_new must be neither x0 nor x_best.  iter >= 0.
 *   nd_square_l2_commit     rows whose flags (nd_square_accept) hold ND_SQUARE_ACTIVE | ND_SQUARE_ACCEPT: x_best = x_new over the whole
 *                           image of per_image = Cin * H * W elements; every other row: nothing.  A rejected candidate is not taken back:
 *                           the next propose rewrites the whole of x_new.
 * The bookkeeping of a query is nd_square_accept, unchanged. */
#define ND_SQUARE_L2_INIT_TAG 0x53324931u
#define ND_SQUARE_L2_STEP_TAG 0x53325331u
#define ND_SQUARE_L2_SIGN_TAG 0x53324731u
#define ND_SQUARE_L2_SUMS 6
#define ND_SQUARE_L2_S_W1 0
#define ND_SQUARE_L2_S_ALL 1
#define ND_SQUARE_L2_S_MASK 2
#define ND_SQUARE_L2_S_OUT 3
#define ND_SQUARE_L2_S_U 4
#define ND_SQUARE_L2_S_NEW 5
size_t nd_square_l2_ws_floats(int Cin, int H, int W);
int nd_square_l2_init(const float *x0_dev, const int64_t *index_dev, const float *eta0_dev, float *x_best_dev, float *x_new_dev,
                      float *sums_dev, float *ws_dev, int B, int Cin, int H, int W, int s0, uint64_t seed, uint32_t restart, float eps,
                      float lo, float hi, void *stream);
int nd_square_l2_propose(const float *x0_dev, const float *x_best_dev, float *x_new_dev, const int64_t *index_dev,
                         const float *margin_min_dev, const float *eta_dev, int32_t *win_dev, float *sums_dev, float *ws_dev, int B,
                         int Cin, int H, int W, int s, int iter, uint64_t seed, uint32_t restart, float eps, float lo, float hi,
                         void *stream);
int nd_square_l2_commit(float *x_best_dev, const float *x_new_dev, const int32_t *flags_dev, int B, size_t per_image, void *stream);

/* ---- the L2 attacks (foolbox 3.x L2BasicIterativeAttack / L2ProjectedGradientDescentAttack) and Carlini & Wagner's L2 attack
 * (L2CarliniWagnerAttack); the listings: nested_diffusion_amd/attack.py.  B images of per_image fp32 elements (per_image % 4 == 0,
 * 1 <= B <= 65535, images 16-byte aligned); every elementwise operation one rounded fp32 op in the listing's order (contraction off).
 * No entry point allocates, copies synchronously or synchronises.  Row reductions use no floating-point atomics: nd_l2_parts(per_image)
 * workgroups per image each write one partial into the workspace, and a finishing pass folds them in a fixed order; the shape
 * depends on per_image alone, so a norm has the same bits on every run and at every batch size.  ws: 2 * ND_L2_MAX_PARTS * B floats
 * (nd_l2_random_start: ND_L2_MAX_PARTS * B).  The per-image norms are written out: exactly the values the elementwise pass used.
 *   nd_margin_head_bwd    Carlini & Wagner's head, beside nd_xent_head_bwd: other [B] int32 = the first maximal index of logits over the
 *                         non-label columns (a NaN logit never wins; no number among them: the first non-label column),
 *                         margin [B] = logits[label] - logits[other] + confidence, dlogits = +consts[b] at the label and -consts[b] at
 *                         other where margin > 0, else 0, dfeat [B, E] = dlogits . head_w ([C, E]): the gradient of
 *                         sum_b consts[b] * max(0, margin[b]).  At margin == 0 the gradient is 0 (torch's maximum would pass half).
 *                         2 <= C <= 1024.  A label outside [0, C): margin NaN, other -1, dfeat 0.
 *   nd_l2_step            gnorm [B] = sqrt(sum g^2); t = x + alpha * (g * (1 / max(gnorm, 1e-12))); d = t - x0;
 *                         dnorm [B] = sqrt(sum d^2) of the fp32 d actually formed; out = clip(x0 + d * min(1, eps / max(dnorm, 1e-12)),
 *                         lo, hi).  A NaN anywhere in a row's gradient (gnorm NaN), or a gnorm that overflows, makes that row take no
 *                         step (t = x), the convention of nd_linf_step.  grad NULL: no step and gnorm (may be NULL) = 0; with
 *                         lo = -inf, hi = inf that is foolbox's final clip_perturbation.
 *   nd_l2_random_start    foolbox's uniform_n_balls start: out = clip(x0 + eps * (z / snorm), lo, hi), z the first n = per_image of
 *                         n + 2 standard normals, snorm [B] = sqrt(sum over all n + 2).  Normal 4q + e of image b comes from
 *                         Philox4x32-10 with key = (seed low word, seed high word) and counter = (first_image + b, q, restart,
 *                         ND_L2_START_TAG), the four words mapped by the Box-Muller of nd_rng (words 0, 1 -> normals 0, 1; words 2, 3
 *                         -> normals 2, 3).  Quads 0 .. per_image / 4 are drawn; the last supplies normals n and n + 1, its other two
 *                         are discarded.  The counter is keyed on the global image index: a sub-batch draws what it draws in the full
 *                         batch.
 *   nd_cw_attack_space    a = (lo + hi) / 2, b = (hi - lo) / 2: w0 = atanhf(((x0 - a) / b) * 0.999999f), xrec = tanhf(w0) * b + a.
 *                         n elements, n % 4 == 0.
 *   nd_cw_model_space     t = tanhf(w0 + delta), x = t * b + a, both stored; sq_rec [B] = sum (x - xrec)^2, sq_x0 [B] = sum (x - x0)^2.
 *   nd_cw_control         one thread per image: adv = argmax(logits + confidence * onehot(label)) != label (the first maximal index, a
 *                         NaN never wins, all NaN: index 0), found |= adv, norm = sqrt(sq_x0), new_best = adv && norm < best_norm,
 *                         best_norm = norm where new_best, flags [B] = new_best, loss [B] = consts * max(0, margin) + sq_rec (a NaN
 *                         margin counts as 0).  found, flags int32 [B].  2 <= C <= 1024.
 *   nd_cw_update          one pass per element: where flags[b] (flags may be NULL), best = x; then
 *                         g = ((dx + 2 * (x - xrec)) * b_half) * (1 - t * t); m = 0.9 m + 0.1 g; v = 0.999 v + 0.001 (g * g);
 *                         delta = delta - (stepsize * (m / bc1)) / (sqrtf(v / bc2) + 1e-8).  bc1 = 1 - 0.9^(k+1), bc2 = 1 - 0.999^(k+1),
 *                         computed by the host in double.  b_half must be the b of nd_cw_model_space, (hi - lo) / 2 formed in fp32
 *                         from the fp32 lo and hi, so that the gradient uses the b that produced x.  No transcendental: sqrtf and
 *                         division only.
 * One CW iteration on a stream is nd_cw_model_space, the margin gradient, nd_cw_control, nd_cw_update. */
#define ND_L2_START_TAG 0x4C325331u
#define ND_L2_MAX_PARTS 256
int nd_l2_parts(size_t per_image);
int nd_margin_head_bwd(const float *logits_dev, const int64_t *labels_dev, const float *consts_dev, const float *head_w_dev,
                       float *dfeat_dev, float *margin_dev, int32_t *other_dev, int B, int C, int E, float confidence, void *stream);
int nd_l2_step(const float *x_dev, const float *x0_dev, const float *grad_dev, float *out_dev, float *gnorm_dev, float *dnorm_dev,
               float *ws_dev, int B, size_t per_image, float alpha, float eps, float lo, float hi, void *stream);
int nd_l2_random_start(const float *x0_dev, float *out_dev, float *snorm_dev, float *ws_dev, int B, size_t per_image, uint64_t seed,
                       uint32_t first_image, uint32_t restart, float eps, float lo, float hi, void *stream);
int nd_cw_attack_space(const float *x0_dev, float *w0_dev, float *xrec_dev, size_t n, float lo, float hi, void *stream);
int nd_cw_model_space(const float *w0_dev, const float *delta_dev, const float *x0_dev, const float *xrec_dev, float *t_dev,
                      float *x_dev, float *sq_rec_dev, float *sq_x0_dev, float *ws_dev, int B, size_t per_image, float lo, float hi,
                      void *stream);
int nd_cw_control(const float *logits_dev, const int64_t *labels_dev, const float *consts_dev, const float *margin_dev,
                  const float *sq_rec_dev, const float *sq_x0_dev, float *best_norm_dev, int32_t *found_dev, int32_t *flags_dev,
                  float *loss_dev, int B, int C, float confidence, void *stream);
int nd_cw_update(float *delta_dev, float *m_dev, float *v_dev, const float *dx_dev, const float *x_dev, const float *xrec_dev,
                 const float *t_dev, float *best_dev, const int32_t *flags_dev, int B, size_t per_image, float stepsize, float bc1,
                 float bc2, float b_half, void *stream);

/* ---- AutoAttack's APGD, L2 (autopgd_base.py attack_single_run with norm = 'L2'; the listing: nested_diffusion_amd/autoattack.py), and the
 * accumulation of an expectation over transformation (nested_diffusion_amd/eot.py); csrc/nd_apgd_l2.hip.  B images of per_image fp32
 * elements (per_image % 4 == 0, 1 <= B <= 65535, images 16-byte aligned), checked before any HIP call, as is a NULL required pointer
 * (ND_ERR_ARG).  Every elementwise operation is one rounded fp32 op in the listed order (contraction off).  No entry point allocates,
 * copies synchronously or synchronises.  n(v)[b] = sqrtf(sum v^2) over image b is the row reduction of the L2 attacks above: grid
 * (nd_l2_parts(per_image), B), per-workgroup partials in the workspace, a finishing pass with the same tree, no floating-point atomics:
 * a norm has the same bits on every run and at every batch size.  ws: 2 * ND_L2_MAX_PARTS * B floats.
 *   nd_apgd_l2_random_start  autoattack's L2 start: out = clip(x0 + eps * (t / (tn + 1e-12)), lo, hi), t per_image standard normals and
 *                            tn = n(t), written to tnorm [B].  Normal 4q + e of row b comes from Philox4x32-10 with key = (seed low
 *                            word, seed high word) and counter = (index[b] (low word), q, restart, ND_APGD_L2_START_TAG), the four
 *                            words mapped by the Box-Muller of nd_rng exactly as in nd_l2_random_start.  Exactly per_image normals are
 *                            drawn (no n + 2 extras: that is foolbox's ball).  index: int64 [B], the GLOBAL image index of each row, so
 *                            a row of a compacted restart subset draws what it draws in the full batch.
 *   nd_apgd_l2_step          the L2 momentum step of one iteration, in place.  Per row b, with xa the row's x_adv on entry, s = step[b]
 *                            and g the row's gradient -- grad_best where flags[b] & ND_APGD_RESTORE, else grad; flags NULL: none (the
 *                            first step, a = 1, with x_adv_old == x_adv; the two may be one buffer):
 *                                g2 = xa - x_adv_old;  x_adv_old = xa
 *                                gn = n(g);            u  = xa + s * (g / (gn + 1e-12))
 *                                d1 = u - x;  n1 = n(d1);  z = clip(x + (d1 / (n1 + 1e-12)) * min(eps, n1), 0, 1)
 *                                v  = (xa + (z - xa) * a) + g2 * (1 - a)
 *                                d2 = v - x;  n2 = n(d2);  x_adv = clip(x + (d2 / (n2 + 1e-12)) * min(eps, n2), 0, 1)
 *                            norms [3, B] receives gn, n1 and n2: exactly the values the elementwise passes used.  Later passes
 *                            recompute the earlier elementwise values instead of storing them (the same bits).  A row whose gn is NaN
 *                            or infinite takes no gradient step (u = xa), the convention of nd_l2_step.  Call order per iteration:
 *                            nd_apgd_control, nd_apgd_update(..., do_step = 0) for the flags' copies and the restore (it writes x_best
 *                            into a restored row's x_adv), then this.
 *   nd_eot_add               acc = acc + g; with divisor > 0, acc = (acc + g) / (float)divisor: one add and one true division, not a
 *                            reciprocal multiply.  n elements, n % 4 == 0, both 16-byte aligned. */
#define ND_APGD_L2_START_TAG 0x41504C32u
int nd_apgd_l2_random_start(const float *x0_dev, const int64_t *index_dev, float *out_dev, float *tnorm_dev, float *ws_dev, int B,
                            size_t per_image, uint64_t seed, uint32_t restart, float eps, float lo, float hi, void *stream);
int nd_apgd_l2_step(const float *x_dev, float *x_adv_dev, float *x_adv_old_dev, const float *grad_dev, const float *grad_best_dev,
                    const int32_t *flags_dev, const float *step_dev, float *norms_dev, float *ws_dev, int B, size_t per_image, float eps,
                    float a, void *stream);
int nd_eot_add(float *acc_dev, const float *g_dev, size_t n, int divisor, void *stream);

/* ---- the gradient through the mapping MLPs (csrc/nd_mlp_grad.hip; the chain: mapping.py GuidingConditioner.input_grad).  The ensemble
 * is conditioned on the mapping networks (patch_embed -> blocks[0..k] -> mlps[k] -> softmax), not on the full ViT's head: these two entry
 * points, with the ViT block gradients above, give the gradient of the conditioners' own loss with respect to the image.  Neither
 * allocates, copies synchronously or synchronises; both are capturable.
 *   nd_linear_bwd         out[M, K] = ((dy[M, N] . W[N, K]) (.) (gate[M, K] > 0)) + add[M, K]: the input gradient of a Linear whose
 *                         [N, K] weight is held as its nd_pack_rows image ONLY (w_packed_dev, ND_DTYPE_F32; read in place, no transposed
 *                         or unpacked copy exists anywhere).  dy, gate, add, out: row-major fp32.  gate may be NULL (no mask); otherwise
 *                         it is the forward's post-ReLU activation and `> 0` is strict: ReLU'(0) = 0 as in torch (+0.0 and -0.0 alike),
 *                         and a NaN gate gives 0.  add may be NULL and may alias out.  1 <= M <= ND_LINEAR_BWD_MAX_M, K % 16 == 0,
 *                         N >= 1; the image's zero rows N .. 16 * ceil(N / 16) meet a dy operand that is zero-filled in registers and
 *                         never read from memory.  An ND_DTYPE_F16 image is refused (ND_ERR_ARG).  No workspace.
 *                         A workgroup owns a range of W's 16-column blocks and walks all row blocks for them: no split over the
 *                         contraction, no atomics, no second pass.  Exact-f32 MFMA (v_mfma_f32_16x16x4_f32); an output element is one
 *                         chain over n whose order depends on (N, K) only, never on M or on which rows share the launch: a row's result
 *                         is bit-identical in any batch and on every run.  A NaN in dy row r reaches out row r only.
 *   nd_ensemble_xent_bwd  the cross-entropy of the members' AVERAGED probabilities.  logits [K, B, C] fp32 (1 <= K <= 32,
 *                         2 <= C <= 1024), labels int64 [B]: p_k = softmax(logits_k) (max-subtracted), P[b, c] = (sum_k p_k[b, c]) / K
 *                         summed in member order k = 0 .. K-1, loss[b] = -logf(P[b, y]), dlogits_k[b, c] = w_k (p_k[b, c] - [c == y]),
 *                         w_k = p_k[b, y] / sum_j p_j[b, y] (the 1 / K cancels).  K == 1 is the plain softmax cross-entropy and is
 *                         formed as a log-softmax, as nn.CrossEntropyLoss is: loss[b] = logf(sum_c exp(l_c - max)) - (l_y - max),
 *                         dlogits[b, c] = p[b, c] - [c == y], no division by p[b, y]: it never reports underflow (a label that trails
 *                         the leading logit by more than 104 gives loss = that margin and dlogits = -1 at the label).  Conventions:
 *                         K >= 2 and sum_j p_j[b, y] == 0 (every member underflows at the label): loss = +inf and dlogits = 0 (a member
 *                         that underflows alone has w_k = 0 exactly, the others share the gradient); a NaN logit anywhere in row b (any
 *                         member; a largest logit of +inf and an all -inf row are such rows): that row's P, loss and dlogits are NaN
 *                         (sign(NaN) = 0 in nd_linf_step: no step); a label outside [0, C): loss NaN, dlogits 0, P as usual.
 *                         labels NULL: only P is written (the scores-only call; loss and dlogits may be NULL). */
#define ND_LINEAR_BWD_MAX_M 128
int nd_linear_bwd(const float *dy_dev, const void *w_packed_dev, const float *gate_dev, const float *add_dev, float *out_dev, int M, int N,
                  int K, int dtype, void *stream);
int nd_ensemble_xent_bwd(const float *logits_dev, const int64_t *labels_dev, float *P_dev, float *loss_dev, float *dlogits_dev, int K, int B,
                         int C, void *stream);

/* ---- training of the mapping MLPs (csrc/nd_mlp_train.hip; the loop: train_mapping.py MappingTrainer; replaces loss.backward() and
 * optimizer.step() of mapping/train_mapping.py:114-115 for the four Linear layers of mapping/models/mlp.py).  With nd_linear_bwd and
 * nd_ensemble_xent_bwd (K = 1: the plain softmax cross-entropy, a log-softmax that is exact at any margin) above, these are the backward pass and torch.optim.Adam of one step.
 * fp32 data and ND_DTYPE_F32 images only (an ND_DTYPE_F16 image is refused, ND_ERR_ARG).  None of them allocates, copies synchronously or
 * synchronises; no atomics, no cross-workgroup communication; every loop is bounded by the shape arguments.
 *   nd_adam_step          what one Adam step needs, formed by the host in double and rounded once: step_size = lr / (1 - beta1^t),
 *                         sqrt_bc2 = sqrt(1 - beta2^t).
 *   nd_linear_wgrad_adam  acc[n, k] = sum_m dy[m, n] x[m, k] (exact-f32 MFMA, v_mfma_f32_16x16x4_f32), then torch 1.10's F.adam listing
 *                         (no weight decay, no amsgrad), one rounded fp32 operation per line, no contraction, correctly rounded division
 *                         and square root, on every fp32 input: denormals are kept (operands of the MFMA, g, g * g, m and v alike), signed
 *                         zeros, infinities and NaN follow IEEE 754 (a zero acc is +0: the contraction starts from +0):
 *                             g = acc * gscale
 *                             m = (m * beta1) + (g * one_minus_beta1)
 *                             v = (v * beta2) + ((g * g) * one_minus_beta2)
 *                             denom = (sqrt(v) / sqrt_bc2) + eps
 *                             w = w - step_size * (m / denom)
 *                         dy [M, N], x [M, K] row-major; w / m / v / g_out: nd_pack_rows images of [N, K] matrices, distinct buffers,
 *                         updated in place.  1 <= M <= ND_LINEAR_BWD_MAX_M, K % 16 == 0, N >= 1.  a == NULL: only g_out is written
 *                         (w / m / v may be NULL); g_out == NULL: no gradient is written; both NULL: ND_ERR_ARG.  Rows of dy / x past M
 *                         are zero-filled in registers, never read; image rows N .. 16 * ceil(N / 16) have gradient exactly 0 and are not
 *                         updated: they stay exactly 0 in w, m, v whatever the step holds (eps = 0 included).  A workgroup owns a range of 16-column blocks, keeps their x fragments in registers and
 *                         walks a range of row blocks: every 16 x 16 block is read and written by exactly one wave, once, and its
 *                         result does not depend on the launch geometry: race-free in place, the same bits on every run.  A NaN in dy
 *                         column n / x column k reaches only weight row n / column k.
 *   nd_linear_wgrad_plan  the launch geometry of that kernel for an [N, K] weight: out[0] = 16-column blocks per workgroup,
 *                         out[1] = workgroups over K, out[2] = workgroups over the row blocks, out[3] = row blocks per workgroup
 *                         (tests pick their shapes and sampled blocks from it).  No GPU needed.
 *   nd_bias_grad_adam     acc[n] = sum_m dy[m, n] in the order m = 0 .. M - 1, then the same listing on b, m, v [N] (g_out [N] or NULL).
 *   nd_unpack_rows        the exact inverse of nd_pack_rows for an ND_DTYPE_F32 image: dst [R, K] row-major, padding rows dropped
 *                         (csrc/nd_pack.hip, beside nd_pack_rows). */
typedef struct nd_adam_step {
    float beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bc2, eps;
} nd_adam_step;
int nd_linear_wgrad_adam(const float *dy_dev, const float *x_dev, void *w_packed_dev, void *m_packed_dev, void *v_packed_dev,
                         void *g_out_packed_dev, int M, int N, int K, int dtype, float gscale, const nd_adam_step *a, void *stream);
int nd_linear_wgrad_plan(int N, int K, int *out4);
int nd_bias_grad_adam(const float *dy_dev, float *b_dev, float *m_dev, float *v_dev, float *g_out_dev, int M, int N, float gscale,
                      const nd_adam_step *a, void *stream);
int nd_unpack_rows(const void *src_packed_dev, float *dst_dev, int R, int K, int dtype, void *stream);

/* ---- training of the ViT (csrc/nd_vit_train.hip; the loop: train_transformer.py ViTTrainer; replaces loss.backward() and
 * optimizer.step() of mapping/train_transformer.py:123-124 for every parameter of timm's vit_base_patch16_224).  The gradients at the
 * activations come from the input-gradient chain above (nd_layernorm_bwd, nd_gelu_bwd_split, nd_attention_bwd, nd_gemm_split on W^T);
 * these three form the gradients at the PARAMETERS and apply torch.optim.AdamW.  fp32 row-major data only.  None of them allocates,
 * copies synchronously or synchronises (they are capturable); no atomics, no split of a contraction over workgroups; every loop is
 * bounded by the shape arguments; the same bits on every run and under any launch geometry.  They differentiate the SUM of the
 * per-image losses (as the chain above does): gscale = 1 / B gives nn.CrossEntropyLoss's mean.  Each has a gradient-only mode
 * (a == NULL: only g_out is written, the parameter and moment pointers may be NULL) and a fused mode (g_out may be NULL); both NULL:
 * ND_ERR_ARG.  In fused mode the parameter, its moments and g_out are distinct buffers.
 *   nd_adamw_step             nd_adam_step's fields plus decay = 1 - lr * weight_decay, all formed by the host in double and rounded
 *                             once.  The update is torch 1.10's F.adamw listing (no amsgrad), one rounded fp32 operation per line, no
 *                             contraction, correctly rounded division and square root:
 *                                 g = acc * gscale
 *                                 w = w * decay
 *                                 m = (m * beta1) + (g * one_minus_beta1)
 *                                 v = (v * beta2) + ((g * g) * one_minus_beta2)
 *                                 denom = (sqrt(v) / sqrt_bc2) + eps
 *                                 w = w - step_size * (m / denom)
 *   nd_gemm_tn_adamw          acc[n, k] = sum_m dy[m, n] x[m, k] (exact-f32 MFMA, v_mfma_f32_16x16x4_f32), then the listing on the
 *                             row-major w, m, v [N, K] in place (g_out [N, K] or NULL).  dy [M, N], x [M, K] row-major, read in the
 *                             lane layout the instruction wants (no transpose).  M >= 1 (thousands of rows: a workgroup owns one tile
 *                             of the result and walks M through LDS stages), N >= 1, K % 16 == 0.  Each element is ONE fma chain over
 *                             m = 0 .. M - 1 carried through every stage: its bits depend on (M, dy, x) alone.  Rows past M and tile
 *                             rows / columns past N / K are zero operands in registers, never read and never written.
 *   nd_gemm_tn_plan           the tile geometry of that kernel for an [N, K] result: out[0] = tile rows (over N), out[1] = tile columns
 *                             (over K), out[2] = rows of M per LDS stage, out[3] = workgroups over K, out[4] = workgroups over N; tile
 *                             (by, bx) covers rows [by * out[0], ...) x columns [bx * out[1], ...).  No GPU needed.
 *   nd_colsum_adamw           acc[n] = sum_m dy[m, n], then the listing on b, m, v [N] (g_out [N] or NULL): biases, pos_embed (dy viewed
 *                             as [B, tokens * E]) and cls_token.  Summation order, a function of M alone: the rows are cut into chunks
 *                             of ND_COLSUM_CHUNK (the last one shorter); a chunk's partial is p = 0, p += dy[r, n] in row order; the
 *                             result is acc = 0, acc += p in chunk order.
 *   nd_layernorm_wgrad_adamw  dgamma[c] = sum_r g[r, c] xhat[r, c], dbeta[c] = sum_r g[r, c] for y = xhat * gamma + beta, g = dL/dy,
 *                             then the listing on gamma and beta with their moments.  xhat = ((x - mean) - cm) * rstd is recomputed
 *                             from x exactly as nd_layernorm / nd_layernorm_bwd compute it; dim % 4 == 0, 4 <= dim <= 2048.  The same
 *                             chunked order over the rows (each product rounded before it is added).  A row's statistics need the
 *                             whole row, so the work is cut over the rows, not the columns: one wave per chunk writes the chunk's
 *                             partials to ws_dev (caller-owned, nd_layernorm_wgrad_workspace_bytes(rows, dim) bytes, 16-byte aligned,
 *                             overwritten; too small: ND_ERR_ARG), a second launch adds them in chunk order and updates.
 *   nd_layernorm_wgrad_workspace_bytes   2 * dim floats per chunk; 0 for a shape the entry point refuses.  No GPU needed. */
#define ND_COLSUM_CHUNK 64
typedef struct nd_adamw_step {
    float beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bc2, eps, decay;
} nd_adamw_step;
int nd_gemm_tn_adamw(const float *dy_dev, const float *x_dev, float *w_dev, float *m_dev, float *v_dev, float *g_out_dev, int M, int N, int K,
                     float gscale, const nd_adamw_step *a, void *stream);
int nd_gemm_tn_plan(int N, int K, int *out5);
int nd_colsum_adamw(const float *dy_dev, float *b_dev, float *m_dev, float *v_dev, float *g_out_dev, int M, int N, float gscale,
                    const nd_adamw_step *a, void *stream);
int nd_layernorm_wgrad_adamw(const float *x_dev, const float *g_dev, float *gamma_dev, float *beta_dev, float *m_gamma_dev, float *v_gamma_dev,
                             float *m_beta_dev, float *v_beta_dev, float *g_out_gamma_dev, float *g_out_beta_dev, int rows, int dim, float eps,
                             float gscale, const nd_adamw_step *a, void *ws_dev, size_t ws_bytes, void *stream);
size_t nd_layernorm_wgrad_workspace_bytes(int rows, int dim);

/* ---- training of the noise estimators (csrc/nd_diffusion_train.hip; the loop: train_diffusion.py NoiseEstimatorTrainer; replaces
 * noise_estimator(...) in train mode, loss.backward(), clip_grad_norm_ and optimizer.step() of
 * diffusion/classification_train_separately.py:967-1006 for latent_model.py's ConditionalModel, arch 'linear').  The Linear layers run on
 * nd_linear, nd_linear_bwd and the gradient-only mode of nd_linear_wgrad_adam / nd_bias_grad_adam above; these entry points are what the
 * model has beyond them.  fp32 row-major data.  None of them allocates, copies synchronously or synchronises; no atomics; every loop is
 * bounded by the shape arguments; the same bits on every run.  Each line of nd_qsample, nd_mse_grad, nd_sumsq, nd_clip_adam and nd_clip_adam_ema is one
 * rounded fp32 operation, no contraction, division and square root correctly rounded; the optimizer listing is nd_linear_wgrad_adam's
 * (csrc/nd_optim.hpp), not a second copy.  The two BatchNorm entry points read and write fp32 and carry a column's statistics and sums
 * in DOUBLE, rounding once where a value is stored (torch's CPU BatchNorm accumulates float data in double too): with few rows that
 * nearly coincide rstd approaches 1 / sqrt(eps) and the backward cancels, and an all-fp32 chain was measured at twelve times torch's error.
 *   nd_bn_train_fwd   ConditionalLinear's gain (latent_model.py:103-104), nn.BatchNorm1d in training mode, the activation and the product
 *                     y = x * y of latent_model.py:177, for u [M, N] = the Linear's output.  One thread owns a column and walks its rows
 *                     r = 0 .. M - 1 in order (M <= 128 makes a reduction across threads pointless; the accesses are coalesced across
 *                     columns).  v is an fp32 product, as torch's separate multiply gives it; the lines after it are double:
 *                         v = fp32(table[t[r]][n] * u[r][n])             (table [rows_table, N], t [M] int32; both NULL: v = u)
 *                         mean = (sum_r v) / M
 *                         var = (sum_r (v - mean) * (v - mean)) / M      (two passes)
 *                         rstd = 1 / sqrt(var + eps)
 *                         xhat = fp32((v - mean) * rstd)
 *                         z = fp32((xhat * gamma[n]) + beta[n])
 *                         a = softplus(z) (ND_ACT_SOFTPLUS: nd_linear's fp32 softplus, threshold 20) or z (ND_ACT_NONE)
 *                         out = a * mul[r][n]                            (fp32; mul [M, N] or NULL: out = a)
 *                     writes out [M, N], xhat [M, N], rstd [N] = fp32(rstd); running_mean / running_var [N], when not NULL, are updated
 *                     in place as torch does: rm = fp32(((1 - mom) * rm) + (mom * mean)), rv = fp32(((1 - mom) * rv) + (mom * (var * (M /
 *                     (M - 1))))).  2 <= M <= ND_LINEAR_BWD_MAX_M (M = 1 is ND_ERR_ARG: torch raises there too), N >= 1 with no
 *                     alignment demand.  A row whose t[r] lies outside [0, rows_table) reads no table row: its v is 0.
 *   nd_bn_train_bwd   the gradient of all of that, given dout [M, N] = dL/dout and the forward's u, xhat, rstd (the fp32 values it
 *                     stored).  Per column, rows in order, z and a recomputed from xhat, gamma, beta exactly as the forward does; the
 *                     sums and dv in double, every output rounded to fp32 once:
 *                         da = dout * mul                                (or dout);   dmul = fp32 dout * a   (written when dmul != NULL)
 *                         dz = da * (1 / (1 + exp(-z)))                  (softplus with z <= 20; otherwise dz = da)
 *                         dgamma = sum_r dz * xhat;   dbeta = sum_r dz
 *                         dv = (gamma * rstd) * ((dz - (dbeta / M)) - (xhat * (dgamma / M)))
 *                         du = dv * table[t[r]][n];   dtable[t[r]][n] = fp32(dtable[t[r]][n] + (dv * u))   (without gain: du = dv)
 *                     dtable [rows_table, N] is the DENSE gradient of the embedding table (nn.Embedding is not sparse here: Adam moves
 *                     every row on every step); the entry point zeroes it on the stream first, and a column's owner adds the rows that
 *                     share a timestep in row order: deterministic.  A row whose t[r] lies outside [0, rows_table) reads and writes
 *                     no table row (du = 0 there).  Outputs are distinct buffers and none of them an input.
 *   nd_qsample        q_sample (diffusion_utils.py:39-50) with PER-ROW coefficients the host gathered from its schedule tables (no
 *                     device-side indexing by t): yt = ((ca[r] * y0) + ((1 - ca[r]) * yhat)) + (cb[r] * e); y0, yhat, e, yt [M, C].
 *   nd_mse_grad       loss[0] = (sum_i (e[i] - out[i])^2) / (M * C), i in row-major order from 0 (one thread), and
 *                     dout = (out - e) * (2 / (M * C)): (e - out).square().mean() and its gradient.  C <= ND_MSE_MAX_C.
 *   nd_sumsq          acc[0] = sum_i x[i] * x[i] (accumulate != 0: added to acc[0]) over n floats, two stages through ws_dev
 *                     (nd_sumsq_workspace_bytes(n), overwritten).  The order is a function of n alone: x is cut into chunks of
 *                     ND_SUMSQ_CHUNK; in a chunk, thread j of 256 forms p = 0, p += x[k] * x[k] for k = chunk start + j + 256 i,
 *                     i = 0 .. 15 (elements past n skipped); the 256 values are added as s[j] += s[j + h] for h = 128, 64 .. 1; the
 *                     chunk totals go to ws.  Then thread j forms p = 0, p += ws[c] for c = j, j + 256, ..., the same tree follows, and
 *                     acc[0] = acc[0] + total (or total).  clip_grad_norm_ takes the norm of the per-tensor norms; summing the squares
 *                     of every tensor into one scalar and taking ONE square root is the same number up to rounding.
 *   nd_sumsq_plan     out[0] = chunks, out[1] = the longest serial chain of additions of that order (tests bound the error by it).  No GPU.
 *   nd_clip_adam      clip_grad_norm_'s scaling and torch.optim.Adam on materialised gradients, elementwise over n floats of w, m, v, g
 *                     (any layout: nd_pack_rows images and row-major tensors alike; the zero padding of an image stays 0 for eps > 0):
 *                         total = sqrt(sumsq[0])
 *                         c = max_norm / (total + 1e-6)
 *                         coef = (c < 1) ? c : 1                         (a NaN gives 1, as torch 1.10's `if clip_coef < 1`)
 *                         g' = g * coef
 *                     then nd_linear_wgrad_adam's listing on (w, m, v, g').  sumsq == NULL: no clipping (g' = g).
 *   nd_clip_adam_ema  the same pass with the EMA shadow of w updated from the new weight (declared and described below nd_clip_adam). */
#define ND_SUMSQ_CHUNK 4096
#define ND_SUMSQ_MAX_N ((size_t)1 << 40)
#define ND_MSE_MAX_C 1024
int nd_bn_train_fwd(const float *u_dev, const float *table_dev, const int32_t *t_dev, int rows_table, const float *mul_dev,
                    const float *gamma_dev, const float *beta_dev, float *out_dev, float *xhat_dev, float *rstd_dev, float *running_mean_dev,
                    float *running_var_dev, int M, int N, int act, float eps, float momentum, void *stream);
int nd_bn_train_bwd(const float *dout_dev, const float *u_dev, const float *table_dev, const int32_t *t_dev, int rows_table,
                    const float *mul_dev, const float *xhat_dev, const float *rstd_dev, const float *gamma_dev, const float *beta_dev,
                    float *du_dev, float *dmul_dev, float *dgamma_dev, float *dbeta_dev, float *dtable_dev, int M, int N, int act,
                    void *stream);
int nd_qsample(const float *y0_dev, const float *yhat_dev, const float *e_dev, const float *ca_dev, const float *cb_dev, float *yt_dev, int M,
               int C, void *stream);
int nd_mse_grad(const float *out_dev, const float *e_dev, float *dout_dev, float *loss_dev, int M, int C, void *stream);
int nd_sumsq(const float *x_dev, size_t n, float *acc_dev, int accumulate, void *ws_dev, size_t ws_bytes, void *stream);
int nd_sumsq_plan(size_t n, size_t *out2);
size_t nd_sumsq_workspace_bytes(size_t n);
int nd_clip_adam(float *w_dev, float *m_dev, float *v_dev, const float *g_dev, size_t n, const float *sumsq_dev, float max_norm,
                 const nd_adam_step *a, void *stream);
/* nd_clip_adam with the exponential moving average of the parameters riding in the same pass (diffusion/ema.py EMA.update after
 * optimizer.step(), classification_train_separately.py:1006-1011): nd_clip_adam's listing on (w, m, v, g), unchanged, then on the NEW weight
 *     pw = one_minus_mu * w
 *     ps = mu * s
 *     s = pw + ps
 * three rounded fp32 operations, no contraction, denormals kept (torch's two scalar products and their sum).  nd_ema_step is formed by the
 * host in double and each field rounded once: one_minus_mu = (float)(1.0 - mu), which is NOT 1.0f - (float)mu ((float)(1.0 - 0.9999) is
 * 1e-04f, 1.0f - 0.9999f is 1.00016594e-04f).  The shadow s is a fifth buffer of n floats in w's layout: the pass moves nine four-byte
 * streams per element where nd_clip_adam moves seven, and w is not read a second time.  The zero padding of an image stays 0 in s
 * (c1 * 0 + c2 * 0).  float4 accesses when n % 4 == 0 and all five buffers are 16-byte aligned, scalar ones otherwise.  ND_ERR_ARG before
 * any launch: a NULL s or e (or any NULL nd_clip_adam refuses), n < 1, a pointer that is not 4-byte aligned, any two of w, m, v, g, s
 * equal.  No allocation, no synchronisation: capturable like nd_clip_adam. */
typedef struct nd_ema_step {
    float one_minus_mu, mu;
} nd_ema_step;
int nd_clip_adam_ema(float *w_dev, float *m_dev, float *v_dev, const float *g_dev, float *s_dev, size_t n, const float *sumsq_dev,
                     float max_norm, const nd_adam_step *a, const nd_ema_step *e, void *stream);

/* ---- the input gradient of the ensemble, through the sampler (csrc/nd_ensemble_grad.hip; the chain: ensemble_grad.py SamplerTape and
 * EnsembleTarget).  The reference has the hook and never uses it: p_sample(..., output_detach=False), diffusion/diffusion_utils.py:80-83,
 * 103-106, 133-134.  Eval mode, guidance=True, arch 'linear', fp32.  The Linear layers run on nd_linear (scale / shift / softplus epilogue on
 * the folded tables of nd_load_member: z = a_t[n] (W h)[n] + c_t[n]) and nd_linear_bwd above; these entry points are what the chain has
 * beyond them.  Rows are r = trial * B + image, M = B * mc.  None of them allocates, copies synchronously, synchronises or uses atomics; every
 * loop is bounded by the shape arguments; the same bits on every run; all are capturable.  Each listed line is one rounded fp32 operation, no
 * contraction.
 *   nd_cond_mul            y[r][n] = s[r][n] * mul[r % B][n] (latent_model.py:177: y = x * y with x = xe [B, N]); s, y [M, N].  The
 *                          forward's counterpart of the block backward below, a SMALL KERNEL OF ITS OWN, not fused: nd_linear's epilogue
 *                          gives s1 = softplus(a_t (W1 inp) + c_t), the backward needs s1 itself (d xe = sum d1 s1), lin2 reads y1.
 *   nd_cond_act_bwd        the eval-mode backward of one ConditionalLinear + BatchNorm1d + softplus block (latent_model.py:101-105, 174-183;
 *                          also encoder_x.1 / .4 and, with h NULL, norm: latent_model.py:127-135, 155), from the block's taped OUTPUT
 *                          h = softplus(z) [M, N], one scale row a_t [N] (the folded gain of timestep t) and the optional product operand
 *                          mul [B, N]:
 *                              sg = (h > 20) ? 1 : -expm1f(-h)               (= sigma(z); the plain 1 - exp(-h) cancels to 0 for
 *                                                                              z <~ -16; h NULL: sg = 1, no activation)
 *                              g = dh * mul[r % B][n]                         (mul NULL: g = dh)
 *                              du = (g * sg) * a_t[n]
 *                              acc = acc + (dh * h)                           (mul given; acc = 0, then the image's trials in trial order)
 *                              dmul_acc[b][n] = dmul_acc[b][n] + acc          (mul given: the block's owner ADDS to what the buffer held,
 *                                                                              once, after the trials: the T steps accumulate in step order)
 *                          dh, du [M, N] (du may be dh), dmul_acc [B, N].  M >= 1, B >= 1, M % B == 0, N >= 1 with no alignment demand.
 *                          One thread owns one column of one image: a_t[n] and mul[b][n] stay in registers across its trials.  A NaN in
 *                          row r reaches row r of du and its image's dmul_acc only.
 *   nd_reverse_step        one line of p_sample_loop on the [M, C] state, in the reference's operation order (csrc/nd_step.hpp's
 *                          nd_posterior / nd_y0_reparam: the device functions the sampler's own kernels use, not a second copy):
 *                              ND_RSTEP_INIT    out = z + ymean[r % B]                                   (diffusion_utils.py:139-140)
 *                              ND_RSTEP_UPDATE  out = p_sample's posterior(y, ymean, eps, z; alpha_t, s_t, s_tm1)    (:68-92)
 *                              ND_RSTEP_LAST    out = 1 / sqrt(1 - s_t^2) * (y - (1 - sqrt(1 - s_t^2)) * ymean - eps * s_t)    (:99-111)
 *                          y [M, ldy] (its first C columns), eps, z [M, C], ymean [B, C]; alpha_t, s_t = one_minus_alphas_bar_sqrt[t],
 *                          s_tm1 = its entry t - 1 are the host's table entries.  out [M, ldo]: ldo == C, or 2C <= ldo <= 64, the form
 *                          lin1 reads: columns C .. 2C-1 = ymean[r % B] (y_0_hat and y_T_mean are one tensor), the rest 0.
 *   nd_reverse_step_bwd    the backward of one such step.  It is affine in (y_t, y_T_mean, eps): with sab = sqrt(1 - s_t^2) and gamma0..2 of
 *                          diffusion_utils.py:75-78, cy = gamma0 / sab + gamma1, cm = gamma2 - gamma0 (1 - sab) / sab, ce = -gamma0 s_t / sab;
 *                          the last step (t = 0): cy = 1 / sab, cm = -(1 - sab) / sab, ce = -s_0 / sab; the start y_T = z + y_T_mean:
 *                          cm = 1.  The host forms them in double and rounds once (ensemble_grad.reverse_step_coefficients).  g [M, ldg]:
 *                          columns 0 .. C-1 = dL/dy_{t-1}; ldg >= 2C: columns C .. 2C-1 are the yhat half of the gradient at lin1's input.
 *                              deps[r][c] = ce * g[r][c]                      (deps [M, C] or NULL)
 *                              dyadd[r][c] = cy * g[r][c]                     (dyadd [M, lda] or NULL; columns C .. lda-1 are written 0: it
 *                                                                              is the `add` of lin1's nd_linear_bwd)
 *                              acc = acc + (cm * g[r][c]);  acc = acc + g[r][C + c] (ldg >= 2C)      (acc = 0; trials in trial order)
 *                              dymean[b][c] = dymean[b][c] + acc
 *   nd_aggregate_xent_bwd  the ensemble's own loss (classification_train_separately.py:392-398, 425-447): q_s = softmax(-(y0_s - 1)^2 /
 *                          temperature), P = (sum_s q_s) / S summed s = 0 .. S-1 with nd_aggregate's operations (P has nd_aggregate's
 *                          bits), loss[b] = -logf(P[b][y]) formed as -logf(Sy / S), Sy = sum_s q_s[y], and
 *                              w = q_s[y] / Sy;  t = q_s[c] - [c == y];  dsamples[s][b][c] = (w * t) * ((y0 - 1) * -2 / temperature)
 *                          samples, dsamples [S, B, C], 1 <= C <= 16.  Conventions as nd_ensemble_xent_bwd: a label outside [0, C):
 *                          loss NaN, gradient 0, P as usual; a NaN in an image's samples: that image's row of P, its loss and its
 *                          gradients NaN; P[b][y] == 0: loss +inf, gradient 0.  labels NULL: P only (loss and dsamples may be NULL).
 *   nd_softmax_bwd         dlogits[r][c] = p[r][c] * (dp[r][c] - dot), dot = sum_c dp[r][c] * p[r][c] in class order; p, dp, dlogits
 *                          [rows, C] (the conditions yhat [K, B, C] and their gradient).  dlogits is neither input. */
#define ND_RSTEP_INIT 0
#define ND_RSTEP_UPDATE 1
#define ND_RSTEP_LAST 2
int nd_cond_mul(const float *s_dev, const float *mul_dev, float *y_dev, int M, int N, int B, void *stream);
int nd_cond_act_bwd(const float *dh_dev, const float *h_dev, const float *a_t_dev, const float *mul_dev, float *du_dev, float *dmul_acc_dev,
                    int M, int N, int B, void *stream);
int nd_reverse_step(int mode, const float *y_dev, int ldy, const float *ymean_dev, const float *eps_dev, const float *z_dev, float *out_dev,
                    int ldo, int M, int B, int C, float alpha_t, float s_t, float s_tm1, void *stream);
/* nd_reverse_step's layouts for one step of a sampler plan (nd_set_sampler: strided timesteps, generalized eta update), the taped
 * forward of the ensemble gradient:  out[r][c] = fmaf(cz, z, fmaf(ce, eps, fmaf(cm, ymean[r % B], cy * y)))  -- the device function the
 * sampler's coefficient kernels call, so the bits are theirs.  z_dev may be NULL when cz == 0 (the plan's row 0, or eta = 0): 0 is used
 * for the draw.  Non-finite coefficients are refused.  nd_reverse_step_bwd with the same (cy, cm, ce) is its backward. */
int nd_reverse_step_coef(const float *y_dev, int ldy, const float *ymean_dev, const float *eps_dev, const float *z_dev, float *out_dev,
                         int ldo, int M, int B, int C, float cy, float cm, float ce, float cz, void *stream);
int nd_reverse_step_bwd(const float *g_dev, int ldg, float cy, float cm, float ce, float *deps_dev, float *dyadd_dev, int lda,
                        float *dymean_dev, int M, int B, int C, void *stream);
int nd_aggregate_xent_bwd(const float *samples_dev, const int64_t *labels_dev, float *P_dev, float *loss_dev, float *dsamples_dev, int S,
                          int B, int C, float temperature, void *stream);
int nd_softmax_bwd(const float *p_dev, const float *dp_dev, float *dlogits_dev, int rows, int C, void *stream);

/* ---- input perturbations of the robustness protocol (diffusion/utils.py:272-414; applied at
 * classification_train_separately.py:726-737).  Images are [B, C, H, W] fp32, contiguous. ------------------- */
/* add_noise (:272-279): out = x + z * std, z = the randn_like draw (supplied, like the sampler's noise). */
int nd_img_add_noise(const float *x_dev, const float *z_dev, float *out_dev, size_t n, float std, void *stream);
/* adjust_brightness (:390-399): out = clamp(x + k, 0, 1). */
int nd_img_brightness(const float *x_dev, float *out_dev, size_t n, float k, void *stream);
/* adjust_contrast (:402-414): m = per-image mean; out = clamp(m + (x - m) * k, 0, 1).  mean_ws_dev: B floats. */
int nd_img_contrast(const float *x_dev, float *out_dev, float *mean_ws_dev, int B, size_t per_image, float k, void *stream);
/* torch interpolate(mode='bilinear', align_corners=False) [B,C,Hi,Wi] -> [B,C,Ho,Wo]: down_up_sample (:372-387) is two
 * calls.  With crop_dev != NULL ([B][2] int32 = top, left) the source is the crop_size x crop_size window of each
 * image: random_crop_and_resize (:282-312; torchvision Resize on tensors = the same interpolate).  The source coordinate
 * scale * (dst + 0.5) - 0.5 is one fused multiply-add, as in torch's builds. */
int nd_img_resize_bilinear(const float *x_dev, float *out_dev, int B, int C, int Hi, int Wi, int Ho, int Wo,
                           const int32_t *crop_dev, int crop_size, void *stream);
/* random_cover_new (:315-349): zero n_rects squares of side `side` per image, in place; rects_dev [B][n_rects][2]
 * int32 = (top, left), chosen on the host with the reference's rejection sampling. */
int nd_img_cover(float *x_dev, int B, int C, int H, int W, const int32_t *rects_dev, int n_rects, int side, void *stream);
/* The training input (replaces ImageFolderDataset.__getitem__ + the DataLoader's collate for a device-resident set): one batch
 * out [B][3][pixels] fp32 from the decoded uint8 store [n_images][src_channels][pixels] (src_channels 1: the three planes are equal
 * and stored once; 3: RGB planes): out[b][c][p] = lut[c][store[idx[b]][src_channels == 1 ? 0 : c][p]].  lut_dev [3][256] fp32 is
 * ToTensor's /255 (and Normalize) of every byte value, made on the host with the dataset's own expressions: the kernel does no
 * arithmetic on values.  idx_dev: int32 [B]; a row whose index is outside [0, n_images) reads nothing and writes nothing.
 * out / lut / idx 4-byte aligned; offsets into the store are 64-bit (n_images * src_channels * pixels may pass 2^31). */
int nd_img_gather_u8(const uint8_t *store_dev, long long n_images, int src_channels, int pixels, const int32_t *idx_dev, int B,
                     const float *lut_dev, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NESTED_DIFFUSION_H */
