/* caddy_hip.h -- C ABI of libcaddy_hip.so: the MI355X-native (gfx950) CADDY hot path.
 *
 * Drop-in boundary.  The reference is pure Python, so the "FFI" a maintainer binds is ctypes
 * (see INTEGRATION.md); every entry point takes raw device pointers + sizes and returns an int status
 * (0 = ok, negative = error, text via caddy_last_error()).  Nothing here allocates device memory: the caller hands over
 * one workspace (caddy_workspace_bytes) and the flat parameter / gradient buffers (caddy_param_floats /
 * caddy_trainable_floats floats), laid out per caddy_param_info_get -- tensors at the boundary are in the reference's
 * state_dict format (OIHW fp32, names of /root/reference model/main_model/model.py's state_dict).
 *
 * Each function cites the reference interface it replaces (paths relative to the reference repository).
 */
#ifndef CADDY_HIP_H
#define CADDY_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct caddy_ctx caddy_ctx;

/* Hyper-parameters read by the hot path (model/main_model/model.py:28-38, "Config keys" in SURVEY.md section 8a). */
typedef struct caddy_config {
    int variant;        /* 0: model.main_model.model, 1: model.reduced_model.model (config["model"]["architecture"]) */
    int batch;          /* B: clips per forward (per GPU) */
    int seq_len;        /* T: observations per clip */
    int height, width;  /* frame size, multiples of 16 */
    int stacking;       /* training.batching.observation_stacking */
    int actions;        /* data.actions_count */
    int action_dim;     /* model.action_network.action_space_dimension */
    int hidden;         /* model.dynamics_network.hidden_state_size (128 main / 64 reduced) */
    int use_gumbel, hard_gumbel, use_variations;   /* model.action_network.* */
    float centroid_alpha;                          /* model.centroid_estimator.alpha */
    int perceptual;     /* != 0: the context also holds the VGG19 perceptual loss (training/losses.py:379-491): the workspace grows by the
                           packed VGG19 weights and feature maps, caddy_load_vgg must be called before a caddy_loss_backward with
                           caddy_loss_cfg.perceptual != 0 */
    int ensemble;       /* model.action_network.ensamble_size (model/main_model/model.py:28,47): N action networks `action_network.{0..N-1}.*` in the parameter table; 0 or 1 = one.
                           The caller draws the member of a forward pass (model.py:152 / :358: random.choice) and names it with caddy_set_action_member.  At most CADDY_MAX_ENSEMBLE. */
} caddy_config;
#define CADDY_MAX_ENSEMBLE 8

typedef struct caddy_param_info {
    char name[128];   /* reference state_dict key */
    long offset;      /* float offset into the flat parameter buffer (and, for kind 0, the flat gradient buffer) */
    int ndim;
    int shape[4];
    int kind;         /* 0 trainable parameter, 1 BatchNorm running statistic, 2 non-trainable parameter (centroids) */
} caddy_param_info;

/* Noise drawn by the reference from torch's CPU generator, in its call order; device pointers. */
typedef struct caddy_noise {
    const float* eps_states;      /* (B*T, Da)      action_network.py:45 via :92  (first A call)            */
    const float* eps_dirs;        /* (B, T-1, Da)   action_network.py:45 via :108 (first A call)            */
    const float* gumbel_uniform;  /* (B*(T-1), K)   gumbel_softmax.py:33                                    */
    const float* eps_states_rec;  /* second A call (reconstructed states), model.py:277                     */
    const float* eps_dirs_rec;
} caddy_noise;

/* Loss weights of Trainer.compute_losses (training/trainer.py:494-500).  mi_ema: SmoothMutualInformationLoss state (K*K floats,
 * device) or NULL.  perceptual: loss_weights.perceptual_loss_lambda[_pretraining] (training/trainer.py:283,442) -- the VGG19 term of
 * ParallelPerceptualLoss (training/losses.py:379-491); non-zero requires caddy_config.perceptual and a preceding caddy_load_vgg.
 * perceptual_log: evaluate and report the perceptual losses even when the weight is 0 (the reference always logs them). */
typedef struct caddy_loss_cfg {
    double rec, states, entropy, dir_kl, mi, state_kl, hidden, mi_entropy_lambda;
    float* mi_ema;
    float mi_ema_alpha;
    int update_mi_ema;
    double perceptual;
    int perceptual_log;
    int diagnostics;    /* != 0: also evaluate the logging-only scalars of the reference's loss_info (trainer.py:475-491, :358-375) on the device, into
                           losses_host[CADDY_DIAG_0 ...]: no tensor leaves the GPU and no extra host synchronisation is needed for them */
    int no_sync;        /* != 0: losses_host (PINNED host memory) is filled by an asynchronous copy on the stream and the call returns without waiting for it -- the caller
                           reads it after its own event / stream synchronisation, typically once the NEXT step has been enqueued (reference: the .item() calls of
                           training/trainer.py:503-530 wait for the GPU every step) */
} caddy_loss_cfg;

/* losses_host slots.  CADDY_LOSS_PERCEPTUAL = avg_perceptual_loss, _TERM = loss_component_perceptual_loss (trainer.py:505,512);
 * CADDY_LOSS_PERC_R0 + 6 r = perceptual_loss_r{r}, + 1 + l = perceptual_loss_r{r}_l{l} -- l = 0 equals the resolution's total, exactly as the
 * reference logs it (in-place aliasing at training/losses.py:483-487, which also makes levels 1..4 count twice in the term). */
enum { CADDY_LOSS_TOTAL = 0, CADDY_LOSS_REC, CADDY_LOSS_STATES, CADDY_LOSS_ENTROPY, CADDY_LOSS_DIRKL, CADDY_LOSS_MI,
       CADDY_LOSS_STATEKL, CADDY_LOSS_HIDDEN, CADDY_LOSS_L1_R0, CADDY_LOSS_L1_R1, CADDY_LOSS_L1_R2,
       CADDY_LOSS_PERCEPTUAL = 11, CADDY_LOSS_PERCEPTUAL_TERM = 12,
       CADDY_LOSS_F16_SATURATED = 13,      /* 1.0: a split-f16 forward convolution (model or VGG19) staged |x| > 65504 since the last caddy_f16_saturated poll; it was clamped to the f16
                                              range -- call caddy_f16_saturated(ctx): the reporting layers move to a forward without a range limit */
       CADDY_LOSS_PERC_R0 = 16,
       /* caddy_loss_cfg.diagnostics: samples_entropy, action_distribution_entropy, states_magnitude, hidden_states_magnitude, action_directions_{mean,variance}_magnitude,
        * reconstructed_action_directions_{mean,variance}_magnitude, action_directions_reconstruction_error, reconstructed_action_directions_kl_loss,
        * centroids_mean_magnitude, average_centroids_distance, average_action_variations_norm_l2, action_variations_mean -- in this order */
       CADDY_DIAG_0 = 40, CADDY_DIAG_COUNT = 14, CADDY_LOSS_SLOTS = 56 };

/* Output ids of caddy_get_output: 0..19 = positions of the 20-tuple returned by Model.forward_full_model
 * (model/main_model/model.py:280-286); 100+r = r-th entry of the multi-resolution list (tuple position 1). */
enum { CADDY_OUT_MULTIRES0 = 100 };

const char* caddy_last_error(void);

/* --- parameters: replaces nn.Module.state_dict()/load_state_dict()/parameters() (training/trainer.py:36,80-122) --- */
int caddy_param_count(const caddy_config* cfg);
int caddy_param_info_get(const caddy_config* cfg, int index, caddy_param_info* out);
long caddy_param_floats(const caddy_config* cfg);       /* size of the flat parameter buffer (all kinds) */
long caddy_trainable_floats(const caddy_config* cfg);   /* kind-0 entries come first: [0, trainable) */

/* --- VGG19 weights of the perceptual loss: replaces torchvision.models.vgg19(pretrained=True).features inside Vgg19.__init__
 *     (model/layers/vgg.py:16-34).  The 13 convolutions the reference's slices evaluate (features.0 ... features.28; conv5_2..5_4 are
 *     loaded by torchvision but never run), names / shapes / float offsets per caddy_vgg_param_info_get (kind = 3), OIHW fp32.
 *     caddy_load_vgg packs them into the workspace (frozen: once, not per step); `vgg_flat` is not referenced afterwards. --- */
int caddy_vgg_param_count(void);
int caddy_vgg_param_info_get(int index, caddy_param_info* out);
long caddy_vgg_param_floats(void);
int caddy_load_vgg(caddy_ctx* ctx, const float* vgg_flat);
/* Arithmetic of the wide 3x3 convolutions (DESIGN.md "numerics"):  0 = exact fp32 (v_mfma_f32_32x32x2_f32);  16 = split f16 (hi + lo operands,
 * 3 products on the 16-bit matrix pipe, fp32 accumulate: fp32-class, forward default);  17 = split bf16 (3 products, 2^-16 with the full
 * fp32 exponent range: gradient default);  18 / 19 = single-product f16 / bf16 operands (VGG19 only).  caddy_set_precision: the model's
 * convolutions (forward: 0 | 16, backward: 0 | 17); caddy_set_vgg_precision: the perceptual loss network (forward 0 | 16 | 18, dgrad 0 | 17 | 19). */
int caddy_set_precision(caddy_ctx* ctx, int forward, int backward);
/* on (default): with caddy_config.perceptual and loaded VGG19 weights, a TRAINING-mode forward also runs the ground-truth branch of the
 * perceptual loss (resize + VGG19 features of the observations: independent of the model) on the driver's side stream, concurrently with
 * the model's forward pass; caddy_loss_backward then only runs the reconstruction branch.  off: everything inside caddy_loss_backward. */
int caddy_set_perceptual_prefetch(caddy_ctx* ctx, int on);
/* Evaluation (evaluation/evaluator.py:55,62,193-197: SequenceLossEvaluator(ParallelPerceptualLoss())): after a forward pass, the FULL-RESOLUTION perceptual distance per
 * reconstructed frame and VGG19 level, out_host[l * N + n] = mean |relu{l+1}_1(rec_n) - relu{l+1}_1(gt_n)|, n = b * Trec + t (Trec = T - 1, or T after forward_pretraining),
 * l = 0..4; 5 * N doubles, host memory; waits for the stream.  Position t of the reference's "perceptual_loss/pos_t" = sum_l mean_b out[l][b * Trec + t - off]. */
int caddy_perceptual_per_frame(caddy_ctx* ctx, double* out_host);
/* ... and the per-frame reconstruction / state losses of the same evaluator (evaluator.py:192,194, ObservationsLoss / StatesLoss per sequence position), from the loss-kernel
 * family: l1_host[b * Trec + t] = mean |frame - ground-truth observation[:3]| at full resolution, mse_host[b * T + t] = mean (reconstructed state - state)^2; host memory,
 * either may be NULL; waits for the stream. */
int caddy_sequence_losses_per_frame(caddy_ctx* ctx, double* l1_host, double* mse_host);
int caddy_set_vgg_precision(caddy_ctx* ctx, int forward, int dgrad);
/* --- Dataset evaluation: replaces the frame-quality metrics of evaluation/dataset_evaluator.py:150-170 -- MSE (evaluation/metrics/mse.py), MotionMaskedMSE
 *     (evaluation/metrics/motion_masked_mse.py + motion_mask.py), PSNR (evaluation/metrics/psnr.py), SSIM (evaluation/metrics/ssim.py: piq.ssim), VGGCosineSimilarity
 *     (evaluation/metrics/vgg_cosine_similarity.py) and the inputs of DatasetEvaluator.check_range.  A METRICS context holds no model: frames of height x width, the fused
 *     pass in chunks of max_frames frames; vgg != 0 adds the VGG19 feature network (weights through caddy_load_vgg, arithmetic through caddy_set_vgg_precision).
 *     caddy_metrics_workspace_bytes returns 0 (caddy_last_error) for frames smaller than SSIM's 11 x 11 window after its down-sampling, or, with vgg, sides that are not
 *     multiples of 16.  Destroy with caddy_ctx_destroy. --- */
size_t caddy_metrics_workspace_bytes(int max_frames, int height, int width, int vgg);
caddy_ctx* caddy_metrics_ctx_create(int max_frames, int height, int width, int vgg, void* workspace, size_t bytes);
/* ref / gen: (B, T, 3, height, width) fp32 device tensors (the reference's (bs, observations_count, channels, height, width)); frame n = b * T + t.  out_host (host memory,
 * CADDY_FM_COUNT * B * T doubles): out_host[slot * N + n], N = B * T.  MSE and the motion-masked MSE on the raw values (the motion mask from the REFERENCE frames, 0 at t = 0),
 * PSNR = -10 log10(MSE / range^2 + 1e-8), SSIM of gen / range against ref / range, the VGG19 cosine similarity (mean over relu1_1 .. relu5_1; want_vgg != 0, else NaN) and the
 * per-frame minima / maxima of ref and gen (check_range).  Deterministic: two calls on the same input give bit-identical results.  Waits for the stream. */
int caddy_frame_metrics(caddy_ctx* ctx, const float* ref, const float* gen, int B, int T, float value_range, int want_vgg, double* out_host);
enum { CADDY_FM_MSE, CADDY_FM_MOTION_MSE, CADDY_FM_PSNR, CADDY_FM_SSIM, CADDY_FM_VGG_SIM,
       CADDY_FM_REF_MIN, CADDY_FM_REF_MAX, CADDY_FM_GEN_MIN, CADDY_FM_GEN_MAX, CADDY_FM_COUNT };
/* Breakout platform detector (evaluation/metrics/breakout_platform_position.py, BreakoutPlatformPosition.forward + detect_platform) on a metrics context:
 * obs: (B, T, 3, height, width) fp32 device tensor in [0, 1]; out_host[b * T + t] (host memory, B * T int32) = the left edge of the platform in frame (b, t), or -1.
 * Only channel 0 of row `row` is read (detect_platform reads frame[0, row, x]); a column is in the mask iff lo <= v <= hi (never for NaN), and the LAST column
 * (x = width - 1) counts as outside it (the reference's `idx != width - 1`), so a run reaching the right edge ends at width - 2.  The result is the start of the
 * first run of at least min_run masked columns (the reference: 12, `current_position_length > 11`).  The caller passes the reference's row int(188 / 208 * height)
 * and its fp32 channel-0 bounds 100 / 255 - 0.15 and 200 / 255 + 0.15.  Errors (-2, caddy_last_error): a context not from caddy_metrics_ctx_create, null
 * pointers, row outside [0, height), min_run < 1, width > 4096.  Runs in chunks of max_frames frames; one launch per chunk; deterministic; waits for the stream. */
int caddy_platform_positions(caddy_ctx* ctx, const float* obs, int B, int T, int row, float lo, float hi, int min_run, int* out_host);
/* --- LPIPS of the dataset evaluation (evaluation/metrics/lpips.py:14,33: lpips.LPIPS(net='vgg') per observation, called from evaluation/dataset_evaluator*.py).  An LPIPS
 *     context is a metrics context of its own kind: the VGG16 trunk up to relu5_3 on the library's VGG convolution kernels (arithmetic through caddy_set_vgg_precision, the
 *     per-layer f16 range guard as for VGG19) plus the five learned 1x1 "lin" layers; frames of height x width, both multiples of 16 (else 0 / NULL and caddy_last_error), in
 *     chunks of max_frames frames.  caddy_frame_metrics and caddy_load_vgg refuse an LPIPS context, caddy_frame_lpips and caddy_load_lpips any other.  Destroy with caddy_ctx_destroy. --- */
size_t caddy_lpips_workspace_bytes(int max_frames, int height, int width);                                  /* evaluation/metrics/lpips.py:14 */
caddy_ctx* caddy_lpips_ctx_create(int max_frames, int height, int width, void* workspace, size_t bytes);    /* evaluation/metrics/lpips.py:14 */
/* the network's tensors (evaluation/metrics/lpips.py:14): features.{idx}.weight / .bias of torchvision's vgg16 for the 13 convolutions (idx 0 2 5 7 10 12 14 17 19 21 24 26 28),
 * then lin{l}.model.1.weight (1, C_l, 1, 1), l = 0..4; caddy_load_lpips takes a device buffer laid out by their offsets */
int caddy_lpips_param_count(void);
int caddy_lpips_param_info_get(int index, caddy_param_info* out);
long caddy_lpips_param_floats(void);
int caddy_load_lpips(caddy_ctx* ctx, const float* lpips_flat);
/* evaluation/metrics/lpips.py:33: ref / gen as for caddy_frame_metrics, values in [0, value_range] (the package's normalize=True maps them to [-1, 1], then its scaling
 * layer).  out_host (host memory, 6 * B * T doubles): out_host[n] = LPIPS(ref_n, gen_n), out_host[(1 + l) * N + n] = its term of level l (relu1_2, 2_2, 3_3, 4_3, 5_3):
 * the mean over the pixels of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2.  Deterministic (no float atomics); identical frames give exactly 0.  Waits for the stream. */
int caddy_frame_lpips(caddy_ctx* ctx, const float* ref, const float* gen, int B, int T, float value_range, double* out_host);
/* tests: bit l set = the level-l feature maps of both frames travelled as S16 tensors in some chunk of the last caddy_frame_lpips (evaluation/metrics/lpips.py:33); -1: no LPIPS context */
int caddy_debug_lpips_tap_formats(caddy_ctx* ctx);
/* --- FID of the dataset evaluation (evaluation/metrics/fid.py:140-159, called from evaluation/dataset_evaluator.py:225-250, dataset_evaluator_bair.py:130-150 and
 *     dataset_evaluator_breakout.py:142-163): the 2048 pool_3 features of pytorch_fid/inception.py's InceptionV3([3]) per frame, on the implicit-GEMM convolution, pooling and
 *     resize kernels of csrc/fid.hip.  A FID context is a metrics context of its own kind (every other caddy_frame_* / caddy_load_* entry point refuses it): frames of
 *     height x width in chunks of max_frames; resize != 0 mirrors InceptionV3(resize_input=True) (inception.py:143-147: bilinear, 299 x 299), resize == 0 runs the trunk at the
 *     frame's own size, at least 75 x 75 (else 0 / NULL and caddy_last_error).  The mean / covariance / Frechet distance are host-side fp64 (metrics.py).  Destroy with
 *     caddy_ctx_destroy. --- */
size_t caddy_fid_workspace_bytes(int max_frames, int height, int width, int resize);                                     /* pytorch_fid/inception.py:31-36 */
caddy_ctx* caddy_fid_ctx_create(int max_frames, int height, int width, int resize, void* workspace, size_t bytes);       /* pytorch_fid/inception.py:31-36 */
/* the network's tensors under the names of the pt_inception-2015-12-05 state dict (pytorch_fid/inception.py:13,200-201): per BasicConv2d {block}.{branch}.conv.weight (OIHW) and
 * {block}.{branch}.bn.weight / .bias / .running_mean / .running_var, in graph order (94 convolutions; fc.* and AuxLogits.* are not part of the trunk);
 * caddy_load_fid_inception takes a device buffer laid out by their offsets, folds every eval-mode BatchNorm2d(eps=0.001) into its convolution and packs the weights for both
 * arithmetics.  The buffer is not referenced after the call. */
int caddy_fid_param_count(void);
int caddy_fid_param_info_get(int index, caddy_param_info* out);
long caddy_fid_param_floats(void);
int caddy_load_fid_inception(caddy_ctx* ctx, const float* flat);
/* arithmetic of the Inception convolutions: 16 = split f16 (default; three products, the per-layer f16 range guard moves a layer that met |x| > 65504 to exact fp32) | 0 = exact
 * fp32 MFMA.  The environment's CADDY_PRECISION=exact selects 0 at creation. */
int caddy_set_fid_precision(caddy_ctx* ctx, int forward);
/* evaluation/metrics/fid.py:98-137 (get_activations): frames = n x (3, height, width) planar fp32 in [0, 1] on the device; out_host (host memory) receives n x 2048 doubles.
 * Bit-reproducible, and independent of max_frames: every frame's features depend on that frame alone.  Waits for the stream. */
int caddy_fid_features(caddy_ctx* ctx, const float* frames, int n, double* out_host);
/* tests: the output of block 0..3 of InceptionV3.BLOCK_INDEX_BY_DIM (pytorch_fid/inception.py:24-29: 64, 192, 768 and 2048 channels) for the frames of the LAST chunk of the last
 * caddy_fid_features, NCHW fp32 into a device buffer; caddy_debug_fid_fallback_layers: convolutions the range guard moved to exact fp32 (-1: no FID context) */
int caddy_debug_fid_block(caddy_ctx* ctx, int block, float* dst_nchw);
int caddy_debug_fid_fallback_layers(caddy_ctx* ctx);
/* measurement: on != 0 records events at the stage boundaries of the following chunks; ms5 (nullable) receives the times of the last chunk's input stage, stem, 35 x 35, 17 x 17
 * and 8 x 8 stages (pytorch_fid/inception.py:83-123).  caddy_fid_macs_per_frame: multiply-accumulates of the 94 convolutions for one frame, counted from the graph. */
int caddy_debug_fid_stage_ms(caddy_ctx* ctx, int on, float* ms5);
double caddy_fid_macs_per_frame(int height, int width, int resize);
/* --- Inception Score of the dataset evaluation (evaluation/metrics/inception_score.py:17-65; its call is commented out in evaluation/dataset_evaluator.py:74, so the evaluators
 *     compute it only when weights are configured): per frame the softmax over the 1000 logits of torchvision's inception_v3(transform_input=False).eval() behind a bilinear
 *     299 x 299 resize (inception_score.py:20-22,41-43).  The network is the FID trunk's graph in its torchvision flavour -- no 2 x - 1 on the input, F.avg_pool2d(3, 1, 1) with
 *     count_include_pad=True in the A / C / E blocks (both E blocks average), then the global average, fc = Linear(2048, 1000) as a 1 x 1 implicit-GEMM convolution and the
 *     wave-per-frame softmax of csrc/fid.hip.  An IS context is an evaluation context of its own kind; resize == 0 runs the network at the frame's own size (>= 75 x 75; tests).
 *     The score itself is host-side fp64 (metrics.py).  Destroy with caddy_ctx_destroy. --- */
size_t caddy_is_workspace_bytes(int max_frames, int height, int width, int resize);                                     /* evaluation/metrics/inception_score.py:20-22 */
caddy_ctx* caddy_is_ctx_create(int max_frames, int height, int width, int resize, void* workspace, size_t bytes);       /* evaluation/metrics/inception_score.py:20-22 */
/* torchvision's names (inception_score.py:20): the 94 BasicConv2d of the trunk as for caddy_fid_param_info_get, then fc.weight (1000, 2048) and fc.bias; AuxLogits.* does not run
 * in eval mode and has no entry.  caddy_load_is_inception takes a device buffer laid out by the offsets; it is not referenced after the call. */
int caddy_is_param_count(void);                                       /* evaluation/metrics/inception_score.py:20 */
int caddy_is_param_info_get(int index, caddy_param_info* out);        /* evaluation/metrics/inception_score.py:20 */
long caddy_is_param_floats(void);                                     /* evaluation/metrics/inception_score.py:20 */
int caddy_load_is_inception(caddy_ctx* ctx, const float* flat);       /* evaluation/metrics/inception_score.py:20-21 */
/* arithmetic of the convolutions and of fc: 16 = split f16 (default, with the per-layer f16 range guard) | 0 = exact fp32 MFMA; CADDY_PRECISION=exact selects 0 at creation */
int caddy_set_is_precision(caddy_ctx* ctx, int forward);              /* evaluation/metrics/inception_score.py:42 */
/* inception_score.py:39-44: frames = n x (3, height, width) planar fp32 in [0, 1] on the device; out_host (host memory) receives n x 1000 fp32 probabilities.  Bit-reproducible and
 * independent of max_frames.  Waits for the stream. */
int caddy_is_probabilities(caddy_ctx* ctx, const float* frames, int n, float* out_host);      /* evaluation/metrics/inception_score.py:39-44 */
/* tests and measurement: the logits (frames x 1000 fp32, into a device buffer) of the LAST chunk of the last caddy_is_probabilities; the layers the range guard moved to exact fp32
 * (-1: no IS context); event times of the last chunk's input stage, stem, 35 x 35, 17 x 17, 8 x 8 stages and head (fc + softmax) as caddy_debug_fid_stage_ms; multiply-accumulates
 * of one frame (94 convolutions + fc) */
int caddy_debug_is_logits(caddy_ctx* ctx, float* dst);                /* evaluation/metrics/inception_score.py:42 */
int caddy_debug_is_fallback_layers(caddy_ctx* ctx);                   /* evaluation/metrics/inception_score.py:42 */
int caddy_debug_is_stage_ms(caddy_ctx* ctx, int on, float* ms6);      /* evaluation/metrics/inception_score.py:41-43 */
double caddy_is_macs_per_frame(int height, int width, int resize);    /* evaluation/metrics/inception_score.py:41-42 */
/* --- FVD of the dataset evaluation (evaluation/metrics/fvd.py:67-126,188-226, used through IncrementalFVD by evaluation/dataset_evaluator.py:75,229,251 and the Breakout / BAIR
 *     evaluators): the 400 logits RGB/inception_i3d/Mean:0 of the Kinetics-400 I3D per video, on the 3-D implicit-GEMM convolution, SAME-padded 3-D max pools and legacy bilinear
 *     input stage of csrc/fvd.hip.  An FVD context is an evaluation context of its own kind: videos of `frames` frames of height x width in chunks of max_videos; resize != 0
 *     mirrors fvd.py:49-56 (TF1 resize_bilinear to 224 x 224, align_corners=False, no half-pixel centres), resize == 0 runs the trunk at the frame's own size (the head's (2, 7, 7)
 *     average window is then clipped to the final map and the logits averaged over what remains).  The mean / covariance / Frechet distance are host-side fp64 (metrics.py).
 *     Bad geometry: 0 / NULL and caddy_last_error.  Destroy with caddy_ctx_destroy. --- */
size_t caddy_fvd_workspace_bytes(int max_videos, int frames, int height, int width, int resize);                                     /* evaluation/metrics/fvd.py:49-56,188-190 */
caddy_ctx* caddy_fvd_ctx_create(int max_videos, int frames, int height, int width, int resize, void* workspace, size_t bytes);       /* evaluation/metrics/fvd.py:67-71 */
/* the network's tensors under the TF variable names of the module (evaluation/metrics/fvd.py:67-71; prefix RGB/inception_i3d/ and suffix :0 stripped), in graph order: per unit
 * {unit}/conv_3d/w (DHWIO; info.shape = (KT KH KW, Cin, Cout), dhwio5 (nullable) receives the five sizes) and {unit}/batch_norm/beta, moving_mean, moving_variance;
 * Logits/Conv3d_0c_1x1/conv_3d/w and /b; then (kind 4: optional, 1 when the module has none) the {unit}/batch_norm/gamma of the 57 units.  caddy_load_fvd_i3d takes a device
 * buffer laid out by their offsets, folds every eval-mode batch norm (eps 1e-3) into its convolution and packs the weights for both arithmetics.  Not referenced after the call. */
int caddy_fvd_param_count(void);                                                   /* evaluation/metrics/fvd.py:67-71 */
int caddy_fvd_param_info_get(int index, caddy_param_info* out, int* dhwio5);       /* evaluation/metrics/fvd.py:67-71 */
long caddy_fvd_param_floats(void);                                                 /* evaluation/metrics/fvd.py:67-71 */
int caddy_load_fvd_i3d(caddy_ctx* ctx, const float* flat);                         /* evaluation/metrics/fvd.py:67-71 */
/* arithmetic of the I3D convolutions: 16 = split f16 (default; the per-layer f16 range guard moves a layer that met |x| > 65504 to exact fp32) | 0 = exact fp32 MFMA.  The
 * environment's CADDY_PRECISION=exact selects 0 at creation. */
int caddy_set_fvd_precision(caddy_ctx* ctx, int forward);
/* evaluation/metrics/fvd.py:106-126,207-226 (create_id3_embedding): videos = n x (frames, 3, height, width) planar fp32 in [0, 1] on the device; out_host (host memory) receives
 * n x 400 doubles.  Bit-reproducible, and independent of max_videos: a video's logits depend on that video alone.  Waits for the stream. */
int caddy_fvd_embeddings(caddy_ctx* ctx, const float* videos, int n, double* out_host);
/* multiply-accumulates of the 57 convolutions + logits for one video, counted from the graph (evaluation/metrics/fvd.py:67-126) */
double caddy_fvd_macs_per_video(int frames, int height, int width, int resize);
/* tests: the outputs of Conv3d_2c_3x3, Mixed_3c, Mixed_4f, Mixed_5c (block 0..3; 192, 480, 832, 1024 channels) for the videos of the LAST chunk of the last caddy_fvd_embeddings,
 * NCDHW fp32 into a device buffer (evaluation/metrics/fvd.py:118-125 runs the same graph); caddy_debug_fvd_fallback_layers: convolutions the range guard moved to exact fp32
 * (-1: no FVD context) */
int caddy_debug_fvd_block(caddy_ctx* ctx, int block, float* dst_ncdhw);
int caddy_debug_fvd_fallback_layers(caddy_ctx* ctx);
/* measurement: on != 0 records events at the stage boundaries of the following chunks; ms5 (nullable) receives the times of the last chunk's input stage (fvd.py:49-56), stem,
 * Mixed_3, Mixed_4 and Mixed_5 + head */
int caddy_debug_fvd_stage_ms(caddy_ctx* ctx, int on, float* ms5);
/* --- Device-side frame pipeline (csrc/frames.hip): the distinct decoded uint8 RGB frames of one batch in, the model's observation tensor out.  Replaces, on the device, the
 *     host's per-frame crop -> bilinear resize -> normalise (dataset/transforms.py:13-30,90-107) and the channel-concatenating / stacking collate (dataset/batching.py:97-112).
 *     The arithmetic is PIL's 8-bit Image.crop(box) + Image.resize(size, BILINEAR), bit for bit: per axis the triangle filter of support max(in / out, 1), its weights
 *     normalised in double and quantised to 22 fractional bits, out = clip8((2^21 + sum pixel * kk) >> 22), horizontal pass first with a uint8 intermediate, a pass skipped
 *     when its axis keeps its size; the tables are built once on the host at creation.  A FRAMES context is an evaluation context of its own kind (no model, no weights):
 *     source frames of src_h x src_w, crop4 = {left, upper, right, lower} or NULL for the whole frame, output frames of out_h x out_w, at most max_frames source frames per call.
 *     lut512 (host memory): 2 x 256 floats, the value of every byte under mode 0 (((x / 255) - 0.5) / 0.5, transforms.py:99-102) and mode 1 (x / 255, transforms.py:67-87),
 *     computed by the caller with the host's own expression so that the result equals the host path's by construction.  caddy_frames_workspace_bytes returns 0
 *     (caddy_last_error) for a crop box that is not inside the source frame (PIL would pad with black) or a geometry whose single output row does not fit the kernel's LDS.
 *     Destroy with caddy_ctx_destroy. --- */
size_t caddy_frames_workspace_bytes(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w);                                       /* dataset/transforms.py:13-30 */
caddy_ctx* caddy_frames_ctx_create(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w, const float* lut512, void* workspace, size_t bytes);   /* dataset/transforms.py:90-107 */
/* tests: the host copies of the filter tables of axis 0 (horizontal) / 1 (vertical): *ksize taps per output, bounds = out x (first source index, tap count), kk = out x ksize
 * quantised weights (each nullable).  Returns 1 when the kernel runs that pass, 0 when the axis keeps its size and the pass is skipped, -2 on error. */
int caddy_frames_tables_get(caddy_ctx* ctx, int axis, int* ksize, int* bounds, int* kk);                                                                 /* dataset/transforms.py:13-30 */
/* tests: plan5 receives the output rows per workgroup, the most source rows one workgroup keeps, the source rows staged per round of the horizontal pass, the LDS bytes
 * used and the LDS bytes of the kernel variant chosen */
int caddy_debug_frames_plan(caddy_ctx* ctx, int* plan5);
/* frames = (n_frames, src_h, src_w, 3) uint8 on the device, 4-byte aligned; slot_src = n_slots int32 on the device; out = (n_slots, 3, out_h, out_w) planar fp32 on the device:
 * plane triple i is frame slot_src[i] cropped, resized and mapped through the table of `mode`.  Viewed as (bs, T, 3 S, out_h, out_w), slot i is (b, t, s) in row-major order,
 * newest frame first (dataset/video_dataset.py:131-137, dataset/batching.py:97-112).  A slot whose source lies outside [0, n_frames) reads nothing and is filled with NaN.
 * One launch on the context's stream; waits for nothing, allocates nothing, deterministic.  Errors (-2, caddy_last_error): a context of another kind, null or misaligned
 * pointers, n_frames > max_frames, n_frames or n_slots < 1, mode other than 0 or 1. */
int caddy_frames_to_observations(caddy_ctx* ctx, const unsigned char* frames, int n_frames, const int* slot_src, int n_slots, int mode, float* out);    /* dataset/batching.py:97-112 */
/* The frame writer, the output side of the same context (an identity geometry, src = out and no crop, serves callers that have no source frames): fp32 planar frames in, uint8
 * interleaved frames out -- on the device what the host does to every roll-out before it writes PNGs (evaluation/evaluation_dataset_builder.py:60-81,140-153: pad with the first
 * ground-truth frame, (x + 1) / 2 when the minimum is negative, * 255, astype(uint8)) and to every played frame (play.py:140).
 *   rec = (B, Trec, 3, out_h, out_w) fp32 on the device, contiguous.  first (nullable) = B planar 3 x out_h x out_w frames, frame b at first + b * first_stride floats (so it may
 *   point at channels 0..2 of t = 0 of a (B, T, 3 S, H, W) observation tensor); when given it is sequence position 0 and T = Trec + 1, else T = Trec.
 *   out_u8 (nullable) = (B, T, out_h, out_w, 3) uint8; out_f32 (nullable) = (B, T, 3, out_h, out_w) fp32 holding the context's mode-1 table value (x / 255) of every byte, i.e.
 *   evaluation_transform of the PNG the host path would have written.  At least one of the two.
 *   map: 0 = the values are in [0, 1] already; 1 = (x + 1) / 2 (play.py:140); 2 = the builder's rule (evaluation_dataset_builder.py:140-153), (x + 1) / 2 only if the minimum over
 *   all B * T frames, `first` included, is negative -- decided on the device by a reduction launch whose flags the writer launch reads; a NaN anywhere means no mapping (torch.min
 *   returns NaN and NaN < 0 is false), -0.0 is not negative.
 *   Arithmetic, each operation rounded to fp32 and nothing contracted: v = x or (x + 1.0f) * 0.5f; s = v * 255.0f; byte = (int)s for 0 <= s < 256.  Where the host's cast is
 *   undefined the byte saturates: s < 0 -> 0, s >= 256 -> 255, NaN -> 0, and the value is counted.
 * One launch for map 0 and 1, two for map 2, on the context's stream; waits for nothing, allocates nothing, deterministic.  Errors (-2, caddy_last_error): a context of another
 * kind, a null rec, pointers that are not 4-byte aligned, both outputs null, B or Trec < 1, B * T > max_frames, first_stride < 3 out_h out_w with B > 1, map outside 0..2. */
int caddy_frames_write(caddy_ctx* ctx, const float* rec, int B, int Trec, const float* first, long first_stride, int map, unsigned char* out_u8, float* out_f32);    /* evaluation/evaluation_dataset_builder.py:60-81 */
/* stats3 (host memory) receives, for the last caddy_frames_write: whether the values were mapped (1 / 0), the values that saturated (s < 0 or s >= 256) and the NaNs, over
 * all 3 out_h out_w B T values.  Waits for the stream. */
int caddy_frames_write_stats_get(caddy_ctx* ctx, unsigned* stats3);                                                                                                  /* evaluation/evaluation_dataset_builder.py:140-153 */
/* --- Evaluation example sheets (csrc/sheets.hip): the contact sheets the reference's evaluator saves first (evaluation/evaluator.py:115-147), composed on the device from the
 *     fp32 tensors of the forward pass; only the finished image is left to copy.  A SHEETS context is an evaluation context of its own kind (no model, no weights) sized by the
 *     largest sheet a call may ask for: max_rows rows of cells (two per drawn sequence) of max_cols cells (the sequence length).  Destroy with caddy_ctx_destroy.
 *     Layout (torchvision make_grid(list, nrow = T, padding = 2, pad_value = 1)): R rows of T cells of h x w; the image is (R (h + 2) + 2, T (w + 2) + 2, 3) uint8 interleaved,
 *     cell (r, t) starts at pixel (r (h + 2) + 2, t (w + 2) + 2) and every other pixel is 255. --- */
size_t caddy_sheets_workspace_bytes(int max_rows, int max_cols);                                                                                                     /* evaluation/evaluator.py:115-147 */
caddy_ctx* caddy_sheets_ctx_create(int max_rows, int max_cols, void* workspace, size_t bytes);                                                                       /* evaluation/evaluator.py:115-147 */
/* obs = (B, T, channels, H, W) fp32 on the device, of which channels 0..2 are read; rec = (B, Trec, 3, h, w) fp32 on the device, Trec = T or T - 1, (H, W) = (h, w) times 1, 2 or 4;
 * out_u8 = (2 min(B, 30) (h + 2) + 2, T (w + 2) + 2, 3) uint8 on the device.  Row 2 b is the ground truth of sequence b resized to h x w, row 2 b + 1 its reconstruction; with
 * Trec = T - 1 column 0 of a reconstruction row is the (mapped) ground-truth frame 0 (save_examples, evaluator.py:392-436).
 *   resize: F.interpolate(mode = "bilinear", align_corners = False) as the CPU computes it for these factors: a copy; ((0.25 a + 0.25 b) + 0.25 c) + 0.25 d over the source pixels
 *   (2y, 2x), (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1); the same form over (4y + 1, 4x + 1), (4y + 1, 4x + 2), (4y + 2, 4x + 1), (4y + 2, 4x + 2).  Other ratios are refused.
 *   range (check_and_normalize_range, evaluator.py:378-390): the resized ground truth and the reconstruction are each mapped by (x + 1) / 2 when their minimum over all B sequences
 *   is negative; a NaN anywhere in a tensor means no mapping for it, -0.0 is not negative.  byte = (int)(v * 255.0f) with caddy_frames_write's arithmetic and saturation rules.
 *   weighted != 0 (save_examples_with_weights, evaluator.py:314-376, with the mask of MotionLossWeightMaskCalculator.compute_weight_mask, training/losses.py:604-649, as both
 *   weights; full resolution only): on the unmapped tensors m = 1 at t = 0 and, for t >= 1, m = ((d_0 + d_1) + d_2) + bias with d_c = |gt_t - gt_{t-1}| + |rec'_t - rec'_{t-1}|,
 *   rec'_0 = gt_0 when Trec = T - 1; w = m / max |m| over all B sequences; col = lut768[3 min((int)(w * 256.0f), 255) + c]; v = (double)(x * 0.4f) + col * 0.6 on the mapped frame x;
 *   byte = (int)(v * 255.0).  lut768 = 256 x 3 doubles on the device (matplotlib's viridis table), nullable when weighted = 0.  A NaN or a negative m is reported by
 *   caddy_sheet_stats_get (the reference's assert weights_mask.min() >= 0); the image of such a call is not specified.
 * Two launches (a reduction, then the compose launch that writes every byte of the image once, padding included) on the context's stream; waits for nothing, allocates nothing,
 * deterministic.  Errors (-2, caddy_last_error): a context of another kind, null or misaligned pointers (4 bytes; lut768 8), sizes < 1, channels < 3, Trec not in {T, T - 1},
 * a ratio other than 1, 2 or 4, weighted with (h, w) != (H, W) or a null lut768, more rows or columns than the context was created for. */
int caddy_sheet_examples(caddy_ctx* ctx, const float* obs, int B, int T, int channels, int H, int W, const float* rec, int Trec, int h, int w, int weighted, float bias,
                         const double* lut768, unsigned char* out_u8);                                                                                               /* evaluation/evaluator.py:392-436, 314-376 */
/* frames = (n, T, 3, h, w) fp32 on the device; out_u8 = (n (h + 2) + 2, T (w + 2) + 2, 3) uint8 on the device: one row per sequence, as interpolate.py:102-158 lays its
 * interpolation values out.  map: 0 = the values are in [0, 1] already, 1 = (x + 1) / 2 (caddy_frames_write's maps 0 and 1, the same bytes).  One launch.  Errors as above. */
int caddy_sheet_strip(caddy_ctx* ctx, const float* frames, int n, int T, int h, int w, int map, unsigned char* out_u8);                                              /* interpolate.py:102-158 */
/* stats5 (host memory) receives, for the last sheet: whether the ground truth and the reconstruction were mapped (1 / 0 each; the strip reports its map twice), the values that
 * saturated, the NaNs (over the drawn cells), and whether the mask held a NaN or a negative value (evaluator.py:135).  Waits for the stream. */
int caddy_sheet_stats_get(caddy_ctx* ctx, unsigned* stats5);                                                                                                         /* evaluation/evaluator.py:135 */
/* --- Device-side MJPEG video writer (csrc/video.hip): baseline JPEG files encoded on the device, in place of the reference's VideoSaver.save_video (utils/save_video_ffmpeg.py:
 *     172-198; play.py:192, interpolate.py:147), whose ffmpeg is not available here; the AVI container is written on the host (video_writer.py).  A VIDEO context is an evaluation
 *     context of its own kind (no model, no weights) for frames of H x W (each 1..4096) at `quality` 1..100; a call with more than max_frames frames runs in chunks.  Destroy
 *     with caddy_ctx_destroy.  The file of a frame is byte for byte libjpeg's for that quality, 4:4:4 sampling, the Annex K Huffman tables, one interleaved scan (each MCU one Y,
 *     one Cb, one Cr block) and no restart markers -- what Pillow's Image.save(f, format = "JPEG", quality = q, subsampling = 0, optimize = False) writes.  Marker order: SOI,
 *     APP0 (JFIF 1.01, density unit 0, 1 x 1), two DQT, SOF0, four DHT, SOS, the scan, EOI.  All arithmetic is integer:
 *       tables   scale = q < 50 ? 5000 / q : 200 - 2 q; entry = (base * scale + 50) / 100 clamped to 1..255 (Annex K base tables), computed on the host at creation
 *       colour   (jccolor.c, FIX(x) = (int)(x * 65536 + 0.5))  Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16;
 *                Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16;  Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 *       padding  the last column and the last row replicated up to the next multiple of 8; then - 128
 *       DCT      jfdctint.c (CONST_BITS 13, PASS1_BITS 2): rows with << 2 / DESCALE(., 11), then columns with DESCALE(., 2) / DESCALE(., 15), DESCALE(x, n) = (x + (1 << (n - 1))) >> n
 *       quantise d = table[k] << 3 (k in zigzag order): |c| -> (|c| + (d >> 1)) / d, truncating, the sign restored
 *       entropy  (jchuff.c) diff = DC - the previous MCU's DC of that component within the frame (0 at its first MCU); for a value v: nbits = bit length of |v|, the code of
 *                nbits (DC) or (run << 4) + nbits (AC), then the low nbits bits of (v < 0 ? v - 1 : v); 0xF0 for every 16 zeros of a longer run; EOB (0x00) only when the block
 *                ends in zeros; table 0 for Y, table 1 for Cb and Cr; the scan padded with 1-bits to a byte; every 0xFF byte of the scan followed by 0x00 --- */
size_t caddy_video_workspace_bytes(int max_frames, int H, int W);                                                                                                    /* utils/save_video_ffmpeg.py:172-198 */
caddy_ctx* caddy_video_ctx_create(int max_frames, int H, int W, int quality, void* workspace, size_t bytes);                                                         /* utils/save_video_ffmpeg.py:172-198 */
/* the output capacity no input of n frames of H x W can exceed: n (623 header bytes + 2 ceil(blocks (63 (16 + 10) + 11 + 11) / 8) + 2) with blocks = 3 ceil(H / 8) ceil(W / 8) --
 * an AC symbol is at most 16 + 10 bits, a DC symbol 11 + 11, every byte may be stuffed.  0 (caddy_last_error) for sizes outside 1..4096 or n < 1. */
size_t caddy_video_stream_bound(int n, int H, int W);                                                                                                                /* utils/save_video_ffmpeg.py:172-198 */
/* frames_u8 = (n, H, W, 3) uint8 interleaved RGB on the device (what caddy_frames_write produces; any alignment); out_stream (device, out_capacity bytes) receives n complete
 * files back to back; offsets (device, n + 1 words, 4-byte aligned) receives where each file starts and, last, the total length.  The caller copies the offsets and then
 * out_stream[0, total) only.  Five launches per chunk of max_frames frames on the context's stream; waits for nothing, allocates nothing; the bits meet
 * through atomicOr on zeroed words, which does not depend on the order, so a call is deterministic.  Errors (-2, caddy_last_error): a context of another kind, null pointers,
 * misaligned offsets, n < 1, out_capacity < caddy_video_stream_bound(n, H, W) (nothing is written: never a truncated stream), a bound of 2^32 bytes or more. */
int caddy_video_encode(caddy_ctx* ctx, const unsigned char* frames_u8, int n, unsigned char* out_stream, size_t out_capacity, unsigned* offsets);                    /* utils/save_video_ffmpeg.py:172-198 */
/* tests: the host copies of what the context built (each nullable): the two quantisation tables in natural order, luminance first (128 bytes); the header SOI .. SOS;
 * its length (623) */
int caddy_video_tables_get(caddy_ctx* ctx, unsigned char* qtables128, unsigned char* header, int* header_bytes);                                                     /* utils/save_video_ffmpeg.py:172-198 */
/* --- Device-side PNG writer (csrc/png.hip): the lossless files every driver writes (dataset folders NNNNN.png, the frames of play / interpolate, the evaluator's example sheets)
 *     filtered, deflated and framed on the device, so that only the compressed bytes are left to copy.  A PNG context is an evaluation context of its own kind (no model, no
 *     weights) for images of H x W; a call with more than max_frames images runs in chunks.  Destroy with caddy_ctx_destroy.  The files are not Pillow's bytes: the contract is
 *     the PNG and deflate specifications -- any decoder returns exactly the input, and both checksums hold.  Each file is the 8-byte signature, IHDR (8 bits, colour type 2, no
 *     interlace), one IDAT holding a zlib stream (header 0x78 0x01), IEND.  All arithmetic is integer and every combine is order independent (OR, XOR, integer sums), so a call
 *     is reproducible bit for bit:
 *       filter    bpp = 3, an all-zero row above row 0; filter_mode 0..4 applies that type (None, Sub, Up, Average, Paeth) to every row, CADDY_PNG_FILTER_ADAPTIVE computes all
 *                 five and takes the smallest sum over the row of |byte as int8|, ties to the lower type.  The filtered stream is H rows of 1 + 3 W bytes (the type first).
 *       deflate   the stream is cut at multiples of 16384 bytes and every block is compressed on its own: literals and distance-1 matches of length 3..258, taken greedily
 *                 from the second byte of a run of equal bytes (runs restart at a block's first byte); the block goes out stored, fixed or dynamic, whichever is shortest in
 *                 bytes (ties: stored, then fixed).  Dynamic: code lengths limited to 15 (literal / length, distance) and 7 (code-length code), canonical codes, at least two
 *                 codes of non-zero length per tree as zlib does.  Every block but the last of an image is ended on a byte boundary by an empty stored block (3 zero bits, the
 *                 padding, 00 00 FF FF) unless it ends on one already, so that the blocks' places are a prefix sum of their byte lengths.
 *       checksums Adler-32 of the filtered stream from per-block sums; CRC-32 of the IDAT type and payload from the bytes as written, per piece by table and combined by
 *                 multiplying with x^(8 len) mod P --- */
#define CADDY_PNG_FILTER_ADAPTIVE 5
#define CADDY_PNG_BLOCK 16384
size_t caddy_png_workspace_bytes(int max_frames, int H, int W);
/* filter_mode: 0..4 or CADDY_PNG_FILTER_ADAPTIVE.  NULL (caddy_last_error): sizes below 1, another filter_mode, or a geometry whose bound for one image,
 * caddy_png_stream_bound(1, H, W), passes 2^31 - 1. */
caddy_ctx* caddy_png_ctx_create(int max_frames, int H, int W, int filter_mode, void* workspace, size_t bytes);
/* the output capacity no input of n images of H x W can exceed: n (63 + S + 5 ceil(S / 16384)) with S = H (1 + 3 W) -- a stored block is its bytes and 5 more (one byte of
 * block header and padding, LEN, NLEN) and no block goes out longer than stored; 63 = signature 8 + IHDR 25 + IDAT length, type and CRC 12 + zlib header 2 + Adler-32 4 + IEND
 * 12.  0 (caddy_last_error) for sizes or n below 1, or where one image's bound passes 2^31 - 1. */
size_t caddy_png_stream_bound(int n, int H, int W);
/* frames_u8 = (n, H, W, 3) uint8 interleaved RGB on the device (what caddy_frames_write and the sheets produce; any alignment); out_stream (device, out_capacity bytes) receives
 * n complete files back to back; offsets (device, n + 1 words, 4-byte aligned) receives where each file starts and, last, the total length.  The caller copies the offsets and
 * then out_stream[0, total) only.  Four launches per chunk of max_frames images on the context's stream; waits for nothing, allocates nothing.  Errors
 * (-2, caddy_last_error): a context of another kind, null pointers, misaligned offsets, n < 1, out_capacity < caddy_png_stream_bound(n, H, W) (nothing is written: never a
 * truncated stream), a bound of 2^32 bytes or more. */
int caddy_png_encode(caddy_ctx* ctx, const unsigned char* frames_u8, int n, unsigned char* out_stream, size_t out_capacity, unsigned* offsets);
/* --- Device-side PNG reader (csrc/png_read.hip): the files of a frame folder (NNNNN.png, dataset/video.py: Image.open per frame in a DataLoader worker) parsed, inflated and
 *     unfiltered on the device, so that the compressed bytes cross to the device instead of raw uint8 frames, and the frames appear where caddy_frames_observations reads them.
 *     A PNG-read context is an evaluation context of its own kind (no model, no weights) for images of H x W; a call with more than max_frames images runs in chunks.  Destroy
 *     with caddy_ctx_destroy.  The contract is the bytes: frames_u8 is what Pillow decodes, and a zlib stream is accepted exactly where zlib's inflate accepts it:
 *       parse     signature; IHDR first, 13 bytes, 8 bits, colour type 2, compression 0, filter 0, interlace 0, width and height those of the context; chunks walked to IEND;
 *                 CRC-32 of IHDR, every IDAT and IEND verified (ancillary CRCs are not, as in Pillow); the IDAT payloads, any number of any length, gathered; ancillary chunks and
 *                 PLTE skipped, any other critical chunk refused
 *       inflate   zlib header (CM 8, CINFO <= 7, FCHECK, no FDICT); stored (LEN against NLEN), fixed and dynamic blocks (HLIT <= 286, HDIST <= 30, repeats 16 / 17 / 18 across
 *                 the literal / distance boundary, codes to 15 bits), matches 3..258 at 1..32768 also overlapping; refused: over-subscribed sets, incomplete sets other than one
 *                 single code of length 1, a missing end-of-block code, symbols 286 / 287, distance codes 30 / 31, a distance beyond the bytes produced, block type 3; the
 *                 Adler-32 verified; bytes behind it ignored
 *       unfilter  exactly H (1 + 3 W) bytes, every type byte 0..4; None, Sub, Up, Average, Paeth with bpp = 3 and a zero row above row 0
 *     Safety: every read of the blob is bounded by the end of that file (clamped to offsets[n]; past it zero bits, CADDY_PNG_TRUNCATED), every write by the image's own frame and
 *     workspace slice; a bad file costs its own status word, its frame is zero-filled and the other images decode normally.
 *     The capacity for one image's IDAT bytes is S + ((S + 7) >> 3) + ((S + 63) >> 6) + 11, S = H (1 + 3 W): zlib's deflateBound for parameters other than its defaults
 *     (Pillow sets memLevel 9) and the 6 bytes of the zlib wrapper, which holds Pillow's files at every level and, being above S + 5 ceil(S / 16384) + 6 for every S, what
 *     caddy_png_encode writes; more gives CADDY_PNG_TOO_LARGE --- */
#define CADDY_PNG_OK 0
#define CADDY_PNG_NOT_PNG 1          /* no signature, or no IHDR of 13 bytes behind it */
#define CADDY_PNG_TRUNCATED 2        /* the file ends inside the signature, a chunk or the zlib stream, or before IEND */
#define CADDY_PNG_BAD_CRC 3          /* IHDR, an IDAT or IEND */
#define CADDY_PNG_UNSUPPORTED 4      /* bit depth, colour type, interlace, compression or filter method, an unknown critical chunk */
#define CADDY_PNG_GEOMETRY 5         /* width or height other than the context's */
#define CADDY_PNG_BAD_DEFLATE 6      /* the zlib header or a block is one zlib refuses */
#define CADDY_PNG_BAD_ADLER 7
#define CADDY_PNG_BAD_LENGTH 8       /* the inflated length is not H (1 + 3 W) */
#define CADDY_PNG_BAD_FILTER 9       /* a row's type byte above 4 */
#define CADDY_PNG_TOO_LARGE 10       /* more IDAT bytes than the context's capacity for one image */
/* 0 (caddy_last_error): the geometry limits of caddy_png_ctx_create */
size_t caddy_png_read_workspace_bytes(int max_frames, int H, int W);
caddy_ctx* caddy_png_read_ctx_create(int max_frames, int H, int W, void* workspace, size_t bytes);
/* files (device): n files back to back; offsets (device, n + 1 words, 4-byte aligned): where each starts and, last, the total length -- what caddy_png_encode leaves, so its
 * output decodes without touching the host.  frames_u8 (device, (n, H, W, 3) uint8, any alignment) and status (device, n words, 4-byte aligned, CADDY_PNG_*) receive the result.
 * Offsets that are not monotonic or pass offsets[n] give that image an empty or shortened file (CADDY_PNG_TRUNCATED / CADDY_PNG_NOT_PNG), never a read outside
 * files[0, offsets[n]).  One launch per chunk of max_frames images on the context's stream; waits for nothing, allocates nothing.  Returns 0 when it
 * ran -- the verdicts are in status.  Errors (-2, caddy_last_error; nothing is launched): a context of another kind, null pointers, misaligned offsets or status, n < 1. */
int caddy_png_decode(caddy_ctx* ctx, const unsigned char* files, const unsigned* offsets, int n, unsigned char* frames_u8, int* status);     /* dataset/video.py:136-157 */
/* --- Device-side JPEG reader (csrc/jpeg_read.hip): the files of a frame folder whose frames are .jpg (dataset/video.py:120-126 discovers the extension, Image.open reads
 *     anything) and the frames of the MJPEG files caddy_video_encode writes, parsed, Huffman-decoded, inverse-transformed, upsampled and colour-converted on the device.  A
 *     JPEG-read context is an evaluation context of its own kind (no model, no weights) for images of H x W, each 1..4096; a call with more than max_frames images runs in
 *     chunks.  Destroy with caddy_ctx_destroy.
 *     Accepted: SOI; baseline sequential DCT (SOF0), precision 8, three components, chroma 1x1 and luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), width and height those of the
 *     context; one interleaved scan of the three components in frame order with Ss = 0, Se = 63, Ah = Al = 0; Huffman tables 0..3 per class and 8-bit DQT tables 0..3, any
 *     number of DQT / DHT segments of one or several tables each, redefined at will before SOS (the last definition holds); DRI, 0 included; APPn and COM skipped; 0xFF fill
 *     bytes in front of a marker; bytes behind EOI ignored.  Colour space by libjpeg's rule: a JFIF APP0 means YCbCr; else an Adobe APP14 with transform 1 means YCbCr and with
 *     0 or 2 is refused; with neither, the component ids 'R','G','B' are refused and any other ids mean YCbCr.
 *     Contract: for every accepted file an encoder wrote, frames_u8 is byte for byte what Pillow (libjpeg-turbo) decodes: Image.open(..).convert("RGB").  For handwritten or
 *     mutated streams the arbiter is the arithmetic below (libjpeg's own result there depends on its build: long arithmetic with a range-limit table in C, saturating 16 / 32-bit
 *     lanes in SIMD).  All of it is integer, >> is arithmetic, products and sums are formed on 32-bit two's-complement words (computed on unsigned, so nothing is undefined):
 *       entropy   T.81 F.2.2.  EXTEND(v, s) = v < 2^(s-1) ? v - 2^s + 1 : v.  The DC predictor of every component is 0 at the start of the scan and of every restart interval.
 *                 An AC symbol (r, s): s = 0 and r = 15 is ZRL (16 zeros), s = 0 and any other r ends the block (EOB, as libjpeg reads it); no EOB is needed once index 63 is
 *                 written.  In the scan 0xFF, any further 0xFF, 0x00 is one 0xFF data byte; 0xFF, any further 0xFF, then a byte other than 0x00 is a marker, and the interval
 *                 ends in front of the first of those 0xFF.
 *       restarts  with Ri > 0 the scan is ceil(MCUs / Ri) intervals, between them exactly RSTm with m = k mod 8 for the k-th; every interval is decoded on its own, and its
 *                 bytes must be used up by its MCUs to within the < 8 padding bits (whose value is not checked)
 *       dequant   c[zigzag[k]] = value * table[k]
 *       IDCT      libjpeg's jidctint.c (CONST_BITS 13, PASS1_BITS 2, its twelve FIX_* constants): columns first with DESCALE(., 11), then rows with DESCALE(., 18), + 128,
 *                 clamped to 0..255; DESCALE(x, n) = (x + (1 << (n-1))) >> n
 *       chroma    a plane has the true size cw = ceil(W hs / hmax), ch = ceil(H vs / vmax); samples outside it are never read, neighbours are replicated at its edge.
 *                 h2v1 fancy: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2, first = s[0], last = s[cw-1].
 *                 h2v2 fancy: v[i] = 3 s[r][i] + s[r'][i], r' the row above for an even output row and the row below for an odd one (row -1 := row 0, row ch := row ch-1);
 *                 out[2i] = (3 v[i] + v[i-1] + 8) >> 4, out[2i+1] = (3 v[i] + v[i+1] + 7) >> 4, first column (4 v[0] + 8) >> 4, last (4 v[cw-1] + 7) >> 4
 *       colour    (jdcolor.c) cb, cr = sample - 128; R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *                 each clamped to 0..255
 *     Deliberately stricter than libjpeg, which warns and carries on: see the statuses.  The first cause met decides: the markers in file order up to SOS, then the markers of
 *     the scan (count, order, the one behind the scan), then the intervals in order.
 *     Safety: every read of the blob is bounded by the end of that file (clamped to offsets[n]) and every read of a lane by the end of its interval; past it the bit reader
 *     yields zeros and the first symbol that used one ends the image; every write is bounded by the image's own frame and workspace slice; a bad file costs its own status
 *     word, its frame is zero-filled and the other images decode normally. --- */
#define CADDY_JPEG_OK 0
#define CADDY_JPEG_NOT_JPEG 1          /* no SOI */
#define CADDY_JPEG_TRUNCATED 2         /* the file ends inside a segment, before SOS, or inside the scan: before its last MCU is decoded or with no marker behind the scan */
#define CADDY_JPEG_UNSUPPORTED 3       /* SOF1/2/3/5..15, DAC, DHP, EXP; precision other than 8; 1 or 4 components; other sampling; a scan of fewer components or in another order
                                          (non-interleaved, multiple scans); 16-bit DQT; DNL or height 0; the colour cases above; scan parameters other than 0 / 63 / 0 / 0 */
#define CADDY_JPEG_GEOMETRY 4          /* width or height other than the context's */
#define CADDY_JPEG_BAD_TABLE 5         /* a segment length inconsistent with its content; a byte other than 0xFF where a marker must stand, or SOI / RSTm / TEM / 0xFF 0x00
                                          before SOS; a DQT / DHT / component table id out of range; a referenced table never defined; Huffman counts that over-subscribe the
                                          code space or pass 256 symbols; a second SOF; no SOF before SOS */
#define CADDY_JPEG_BAD_CODE 6          /* a bit pattern that is no code of the table */
#define CADDY_JPEG_BAD_COEFFICIENT 7   /* a DC category above 11; an AC size above 10; a run (ZRL included) that passes index 63; a DC value outside -2048..2047 */
#define CADDY_JPEG_BAD_RESTART 8       /* the number of RSTm markers is not ceil(MCUs / Ri) - 1; they are out of the cyclic order; an interval in front of an RSTm needs more bits
                                          than it has, or leaves whole bytes over */
#define CADDY_JPEG_BAD_SCAN 9          /* whole entropy bytes are left over behind the last MCU; a marker other than EOI follows the scan */
/* 0 (caddy_last_error): max_frames outside 1..65535, H or W outside 1..4096 */
size_t caddy_jpeg_read_workspace_bytes(int max_frames, int H, int W);
caddy_ctx* caddy_jpeg_read_ctx_create(int max_frames, int H, int W, void* workspace, size_t bytes);
/* files (device): n files back to back; offsets (device, n + 1 words, 4-byte aligned): where each starts and, last, the total length -- what caddy_video_encode leaves, so its
 * output decodes without touching the host.  frames_u8 (device, (n, H, W, 3) uint8, any alignment) and status (device, n words, 4-byte aligned, CADDY_JPEG_*) receive the
 * result.  Offsets that are not monotonic or pass offsets[n] give that image an empty or shortened file, never a read outside files[0, offsets[n]).  Three launches per chunk
 * of max_frames images on the context's stream: entropy decoding (one wave per image, one lane per restart interval), IDCT (block-parallel), upsampling
 * and colour (pixel-parallel).  Waits for nothing, allocates nothing.  Returns 0 when it ran -- the verdicts are in status.  Errors (-2, caddy_last_error; nothing is launched):
 * a context of another kind, null pointers, misaligned offsets or status, n < 1. */
int caddy_jpeg_decode(caddy_ctx* ctx, const unsigned char* files, const unsigned* offsets, int n, unsigned char* frames_u8, int* status);    /* dataset/video.py:120-157 */
/* on (default): caddy_start_inference folds every eval-mode BatchNorm of the roll-out path (E, R's non-recurrent blocks, D) into the packed
 * weights / bias of the convolution in front of it, and caddy_generate_next runs the folded graph (LeakyReLU and the residual add in the conv
 * epilogues, the ConvLSTM cells' BatchNorm as a second output of the gate kernel): ~35 fewer launches per frame.  off: one BatchNorm launch per
 * nn.BatchNorm2d as in the training graph.  Only caddy_generate_next is affected (model.py:570-607, eval mode). */
int caddy_set_rollout_fold(caddy_ctx* ctx, int on);
/* Bit-reproducible backward pass (default ON since round 5: two backward passes over the same forward give bit-identical gradients, like the reference's CPU path -- training/
 * trainer.py:575-587 on torch CPU kernels).  The forward pass is always bit-reproducible (fixed-order split-K, action indices!).  on = 0 selects the arrival-order form: the partial
 * sums of under-filled dgrads and of the weight-gradient pixel splits meet through fp32 atomics (run-to-run ~1e-5 relative on the flat gradient, amplified by BPTT through the
 * closed-loop steps); it is < 1 % faster (profiles/r05_experiments.md: slabs + fixed-order folds cost 0.6 / 0.9 ms of the 61.5 / 125.2 ms steps). */
int caddy_set_deterministic(caddy_ctx* ctx, int on);

/* --- context --- */
size_t caddy_workspace_bytes(const caddy_config* cfg);
caddy_ctx* caddy_ctx_create(const caddy_config* cfg, float* params, float* grads, void* workspace, size_t workspace_bytes);
void caddy_ctx_destroy(caddy_ctx* ctx);
int caddy_set_stream(caddy_ctx* ctx, void* hip_stream);
/* Bucketed gradient all-reduce (BASELINE north star: "all-reduce of gradients overlapped with the backward on a side HIP stream").
 * All weights are shared over time, so nothing is final before BPTT reaches t = 0; what IS final once the time loop's backward
 * is done are the dynamics_network (85 % of the bytes) and rendering_network ranges of the flat gradient buffer.  During
 * caddy_loss_backward of a caddy_forward_full graph the hook is called once per range, `stream` being the HIP stream on which those
 * gradients become valid (the caller enqueues its all-reduce behind it); the ranges must not be touched again until the caller has waited
 * for its collective.  The remaining ranges are valid when caddy_loss_backward returns (on the ctx stream), as before. */
typedef void (*caddy_grads_ready_hook)(float* grads, long offset, long count, void* stream, void* user);
int caddy_set_grads_ready_hook(caddy_ctx* ctx, caddy_grads_ready_hook hook, void* user);
/* Native data parallelism: the same three reductions issued from C into RCCL (ncclAllReduce over xGMI) on a communicator owned by the context -- replaces
 * nn.DataParallel's per-step replicate / gather / reduce-add (train.py:67-68).  One process per GPU:
 *   rank 0: caddy_dp_unique_id(id) -> the 256 bytes (TWO ncclUniqueIds) travel to every rank (any out-of-band channel, e.g. a torch.distributed broadcast) ->
 *   every rank: caddy_dp_init(ctx, id, world_size, rank, overlap) [overlap = 1: R / D gradient buckets behind the side stream during the backward] ->
 *   per step: caddy_forward_full, caddy_loss_backward, caddy_allreduce_grads (the rest + join), caddy_adam_step(..., grad_scale = 1 / world_size).
 * One communicator per stream: the first id's communicator carries every collective issued on the context's stream, the second one's (created when overlap = 1) the
 * gradient buckets on the side stream -- each communicator sees one totally ordered sequence of collectives on every rank.  caddy_dp_init blocks until every rank has
 * called it, at most CADDY_DP_INIT_TIMEOUT_S seconds (default 180): then it returns -3 with a message instead of hanging.
 * RCCL is resolved with dlopen at the first call (CADDY_RCCL_LIB, librccl.so of the process, /opt/rocm/lib): caddy_dp_available() says whether one was found. */
int caddy_dp_available(void);
int caddy_dp_unique_id(char* out256);
int caddy_dp_init(caddy_ctx* ctx, const char* id256, int world_size, int rank, int overlap);
int caddy_allreduce_grads(caddy_ctx* ctx);
long caddy_dp_bucket_floats(caddy_ctx* ctx);
int caddy_dp_shutdown(caddy_ctx* ctx);
/* Evaluation samplers (evaluation/action_sampler.py:14,63; evaluation/action_variation_sampler.py:14), consumed mid-forward exactly where
 * model/main_model/model.py:171-173,189-190 call them.  The hook runs stream-ordered on device pointers inside the workspace:
 *   stage 0 (if provides_samples):    write samples (n, K)    given log_probs (n, K)                      [n = batch * (seq_len - 1)]
 *   stage 1 (if provides_variations): write variations (n, Da) given sampled_dirs (n, Da) and the final samples (n, K)
 * hook == NULL clears it.  Affects caddy_forward_full / caddy_forward_pretraining until cleared. */
typedef void (*caddy_sampler_hook)(const float* log_probs, const float* sampled_dirs, float* samples, float* variations,
                                   int n, int K, int Da, int stage, void* user);
int caddy_set_sampler_hook(caddy_ctx* ctx, caddy_sampler_hook hook, void* user, int provides_samples, int provides_variations);
/* Data parallelism (one process per GPU): `hook(ptr, n, user)` must sum the n floats at device pointer `ptr` (inside the
 * workspace) over all ranks, in place, stream-ordered (RCCL all-reduce).  It is called for the centroid-EMA sums
 * (centroid_estimator.py:61-63) during caddy_forward_* and for the K x K joint matrix of the mutual-information loss
 * (losses.py:262) during caddy_loss_backward, which gives both the reference's global-batch semantics (the reference
 * computes them on GPU0 over the gathered batch under nn.DataParallel).  The parameter gradients themselves are reduced by
 * the caller with ONE all-reduce of the flat gradient buffer after caddy_loss_backward. */
int caddy_set_allreduce_hook(caddy_ctx* ctx, void (*hook)(float* device_ptr, int count, void* user), void* user, int world_size);

/* --- Model.forward(batch_tuple, ground_truth_observations_init, gumbel_temperature=...) in full-model mode:
 *     model/main_model/model.py:57-82 -> forward_full_model :84-286.  obs: (B,T,3S,H,W) fp32 device, reference layout.
 *     training != 0: train-mode BatchNorm + centroid EMA + backward tape; 0: eval mode (evaluation/evaluator.py:125).
 *     samples_in / variations_in (nullable): outputs of an evaluation action_sampler / action_variation_sampler. --- */
int caddy_forward_full(caddy_ctx* ctx, const float* obs, int gt_init, float tau, const caddy_noise* noise, int training,
                       const float* samples_in, const float* variations_in);
/* --- Model.forward(batch_tuple, pretraining=True, ...) -> forward_pretraining (model/main_model/model.py:290-468).
 *     Afterwards caddy_get_output ids follow THAT function's tuple (4 = reconstructed hidden states (B,T,Ch,h,w),
 *     5 = hidden states, 6 = selected actions, 7 = logits, 8 = samples, 9 = attention; 10..19 as in full mode; frames have T entries)
 *     and caddy_loss_backward adds the `hidden` term (HiddenStatesLoss, training/trainer.py:313). --- */
int caddy_forward_pretraining(caddy_ctx* ctx, const float* obs, float tau, const caddy_noise* noise, int training,
                              const float* samples_in, const float* variations_in);
int caddy_get_output(caddy_ctx* ctx, int id, void* dst);      /* copy one output, converted to the reference layout */
/* d(loss)/d(output) after caddy_loss_backward, same layout (what autograd holds in `.grad` of a retained output);
 * available for ids 0, 100-102, 2, 3, 4, 6, 8, 9, 10, 12, 15, 16, 18. */
int caddy_get_output_grad(caddy_ctx* ctx, int id, void* dst);

/* --- losses + loss.backward(): training/trainer.py:447-500,585 fused into one pass (L1 multi-resolution, VGG19 perceptual, states MSE,
 *     entropy, direction KL, (smooth) mutual information, action-state KL) followed by BPTT through D, R, E, A.
 *     Gradients land in the flat gradient buffer (reference layout).  losses_host: CADDY_LOSS_SLOTS doubles (host). --- */
int caddy_loss_backward(caddy_ctx* ctx, const caddy_loss_cfg* cfg, double* losses_host);

/* --- optimizer.step(): torch.optim.Adam with L2 weight decay (training/trainer.py:36,586); m, v: trainable floats --- */
int caddy_adam_step(caddy_ctx* ctx, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int step, float grad_scale);
/* Ensemble of action networks (caddy_config.ensemble > 1; model/main_model/model.py:152,274 / :358,456: both A calls of a forward pass use the member drawn with random.choice).
 * caddy_set_action_member names the member of the NEXT forward pass.  The members that were not drawn receive no gradient (`.grad is None` in the reference): caddy_adam_step leaves
 * their moments and weights untouched, as torch.optim.Adam does, and applies the drawn member's range with ITS OWN step count `member_step` (torch keeps `step` per parameter: a member
 * drawn k times has been stepped k times); every other parameter uses `step`. */
int caddy_set_action_member(caddy_ctx* ctx, int member);
int caddy_adam_step_member(caddy_ctx* ctx, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step, int member_step, float grad_scale);
/* The same step with torch.optim.Adam's per-parameter bookkeeping passed explicitly, for BOTH forms of optimizer.zero_grad() (training/trainer.py:584): member_step[k] (one per
 * ensemble member; NULL = only the drawn member, with `step`) and s2h_step (state_to_hidden_state_layer, model.py:41-43) are the bias-correction counts of those ranges; 0 skips a
 * range (its .grad is None: torch >= 2.0's set_to_none default for everything the last backward did not reach), > 0 steps it -- with the real gradient where the last pass produced
 * one (the drawn member; state_to_hidden_state_layer after caddy_forward_pretraining), with a ZERO gradient otherwise (torch < 2.0, the reference's pinned 1.4.0: zero_grad()
 * zero-fills, so a parameter that has had a gradient once keeps being decayed and its moments keep ageing).  The host mirror (trainer.py: training.zero_grad_semantics) keeps the counts. */
int caddy_adam_step_ex(caddy_ctx* ctx, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step, const int* member_step, int s2h_step,
                       float grad_scale);

/* --- play.py roll-out: Model.start_inference (model.py:561-568) / Model.generate_next (model.py:570-607), eval mode.
 *     observation: (3S,H,W); variation: (Da) or NULL (= zeros, noise=False); frame_out: (3,H,W); obs_out: (3S,H,W) or NULL.
 *     observation, frame_out and obs_out must NOT overlap (obs_out = cat[frame, observation[:-3]] is written while observation is read):
 *     an overlapping call is rejected with -2. --- */
int caddy_start_inference(caddy_ctx* ctx);
/* Poll of the f16 range guards (one flag word per convolution layer, sticky on the device until this call reads and clears them; waits for the stream).  Return value: bit 0 -- a
 * split-f16 forward convolution of the model (model/layers/) or of VGG19 (model/layers/vgg.py:20-36) met an input beyond the f16 range (|x| > 65504) since the last poll and clamped
 * it; bit 1 -- a NaN was among them (the clamp made it finite: the loss call of that pass reported a NaN total, as the reference's fp32 arithmetic would have).  The layers that
 * reported -- and only those -- run without a range limit from the next forward pass on (exact fp32 for model layers, split bf16 for VGG19 layers), for the lifetime of the context;
 * caddy_fallback_layers returns how many have moved so far. */
int caddy_f16_saturated(caddy_ctx* ctx);
int caddy_fallback_layers(caddy_ctx* ctx);
int caddy_generate_next(caddy_ctx* ctx, const float* observation, int action, const float* variation, float* frame_out, float* obs_out);

/* --- batched roll-out: n independent sequences advance per call, each as Model.start_inference / Model.generate_next would advance it alone (model/main_model/model.py:561-607;
 *     eval-mode BatchNorm is a per-channel affine map, so nothing couples the sequences).  One graph launch per frame whatever n is.
 *     caddy_start_inference_batch: 1 <= n <= min(caddy_config.batch, 64) (else -2); re-initialises the ConvLSTM memory of sequence slots 0 .. n-1 from the learned initial state,
 *       prepares the folded inference weights as caddy_start_inference does and drops a graph captured for another n.  caddy_start_inference(ctx) is the n = 1 case.
 *     caddy_generate_next_batch (-2 before caddy_start_inference_batch):
 *       observations: (n,3S,H,W) device;  actions: n ints, HOST, each in [0, K) (else -2);  variations: (n,Da) device or NULL (= zeros);
 *       reset: n bytes, HOST, or NULL -- a non-zero byte re-initialises that sequence's memory before this step (one sequence restarts while the others go on);
 *       frames_out: (n,3,H,W) device;  obs_out: (n,3S,H,W) device or NULL, per sequence cat[frame, observation[:-3]] (model.py:605).
 *       observations, frames_out and obs_out are 16-byte aligned and must NOT overlap (rejected with -2, as caddy_generate_next does per buffer).
 *       The host arrays are read before the call returns.  With n > 1 under way caddy_generate_next returns -2.
 *     caddy_rollout_copy_state: ConvLSTM (h, c) of all three cells from sequence slot src to slot dst (both in [0, n), else -2) -- a fork: what an all-actions preview
 *       or a tree of action scripts is built from. --- */
int caddy_start_inference_batch(caddy_ctx* ctx, int n);
int caddy_generate_next_batch(caddy_ctx* ctx, const float* observations, const int* actions, const float* variations, const unsigned char* reset, float* frames_out, float* obs_out);
int caddy_rollout_copy_state(caddy_ctx* ctx, int src, int dst);

/* --- live kernel timing: HIP events recorded on the launch stream around every conv launch between begin and end.
 *     out = CADDY_PROFILE_FAMILIES kernel families (csrc/common.h CK_*: the four k_conv_fwd tilings, k_conv_thin_out, k_conv_thin_in, three
 *             k_conv_wgrad tilings, k_conv_wgrad_small, k_wgrad_thin, k_conv_wgrad_tile, k_conv_narrow, k_conv_hx<128|64|32> on 4 waves, k_wgrad_hx, k_conv_hx<128> on 8 waves)
 *             x {launches, algorithmic FLOPs, total milliseconds, algorithmic bytes} (SURVEY 8d definitions) --- */
#define CADDY_PROFILE_FAMILIES 18
/* test aid: NaN-fill the not-zero-filled (first-touch) part of the gradient arena before every backward pass */
int caddy_debug_set_poison(caddy_ctx* ctx, int on);
/* test aid: caddy_loss_backward stops after the loss kernels, so caddy_get_output_grad returns the gradient of the DIRECT loss terms only
 * (what autograd holds in `.grad` of the stacked output tensors, which the D->E feedback does not read) */
int caddy_debug_set_seeds_only(caddy_ctx* ctx, int on);
int caddy_profile_begin(caddy_ctx* ctx);
int caddy_profile_end(caddy_ctx* ctx, double* out /* 4 * CADDY_PROFILE_FAMILIES doubles */);
/* per-launch records since caddy_profile_begin (call before caddy_profile_end): 7 doubles each
 * {kind 0 fwd / 1 dgrad / 2 wgrad / 3 VGG19 forward / 4 VGG19 dgrad, output pixels, K (padded input channels), Cout, kernel size, algorithmic FLOPs, ms} */
int caddy_profile_records(caddy_ctx* ctx, double* out, int max_records);
/* phase marks recorded on the ctx stream during profiled steps (forward: pack / E on the ground truth / A / teacher-forced steps / closed-loop steps / A on the
 * reconstructions; backward in reverse): names_out = max x 48 bytes, ms_out[i] = time since the previous mark.  Call before caddy_profile_end. */
int caddy_profile_phases(caddy_ctx* ctx, char* names_out, float* ms_out, int max);

/* --- introspection (debug / tests): the i-th intermediate activation (grad=0) or its gradient (grad=1) of the last
 *     forward, converted to (N,C,H,W) --- */
int caddy_debug_count(caddy_ctx* ctx);
/* kernel nodes of the captured per-frame roll-out graph: the launches one graph launch replaces (tools/bench_rollout_batch.py).  0: no graph is captured (the frames run
 * eagerly, or none has run since caddy_start_inference[_batch]); -1: the count is not available */
int caddy_debug_rollout_graph_nodes(caddy_ctx* ctx);
/* BatchNorm fusion bookkeeping since creation: out3 = {train-mode BatchNorm calls, ... whose statistics came from the producing conv's epilogue,
 * ... whose normalised output was never materialised (applied by the consuming convolution)} */
int caddy_debug_fusion_counts(caddy_ctx* ctx, long* out3);
/* tests / A-B: which BatchNorm paths the driver may pick (all default to 1): the one-launch kernel for tiny maps, the lazily applied form, statistics from the conv epilogue */
int caddy_debug_set_bn_paths(caddy_ctx* ctx, int small, int lazy, int epilogue_stats);
/* tests / A-B runs: 0 keeps every VGG19 feature map of the perceptual loss (training/losses.py:379-491, model/layers/vgg.py:20-36) as an fp32 tensor; 1 (default) lets well-filled
 * layers exchange them pre-split for the 16-bit matrix pipe ("S16" tensors, csrc/common.h).  Same convolution results bit for bit; the feature L1 sees hi + lo (2^-22 relative). */
int caddy_debug_set_vgg_s16(caddy_ctx* ctx, int on);
/* tests / A-B runs (round 6): 0 keeps the gradient of every convolution output (the dY of model/layers/residual_block.py:49-68, same_block.py:34-47, up_block.py:31-45,
 * convolutional_lstm_cell.py:92-101) as an fp32 tensor; 1 (default) lets the point-wise backward kernel that produces it write it pre-split (S16-bf16) where the dgrad, the weight
 * gradient and the bias / broadcast-input sums that read it understand the format.  Same matrix operands bit for bit; the column sums see hi + lo (2^-17 relative).
 * caddy_debug_s16_grad_count: how many gradient tensors of the last caddy_loss_backward travelled pre-split. */
int caddy_debug_set_s16_grads(caddy_ctx* ctx, int on);
/* tests / A-B runs (round 6): the VGG19 perceptual loss (training/losses.py:379-491) of a training step is evaluated in `n` chunks of time steps, last steps first, on the side stream
 * beside the BPTT replay, which waits per time step for its chunk; 1 = one pass over all frames before the replay (rounds 2 - 5); 0 = the library's choice
 * (three chunks of the full-resolution level for steps of >= 4 M reconstructed pixels, four from 1 M, else one pass; CADDY_PERC_CHUNKS changes the three, a negative value forces its magnitude).  Takes effect at the next
 * caddy_forward_full.  Same loss; gradients equal up to the summation order of the per-chunk launches. */
int caddy_debug_set_perc_chunks(caddy_ctx* ctx, int n);
/* tests / A-B runs: 1 (default) lets the dgrad launch above a tapped VGG19 map (relu1_1 .. relu4_1 of training/losses.py:379-491), whose epilogue loads the reconstruction's and
 * the ground truth's features for the sign of the L1 seed, also sum |f_rec - f_gt| for the level's loss; 0 = a stand-alone pass over both maps for every level.  Same gradients
 * bit for bit; the level sums are the same fp32 differences added in double in another order.  CADDY_PERC_FUSE_L1 sets the default of new contexts. */
int caddy_debug_set_perc_fuse_l1(caddy_ctx* ctx, int on);
/* tests (nothing is launched): plans the ground-truth VGG19 prefetch of a training forward pass with `trec` reconstructed frames (chunk count: caddy_debug_set_perc_chunks) and walks
 * every (chunk, resolution level) the side stream would run.  out[0] = bytes of the side stream's scratch region, out[1] = bytes the largest walk needs, out[2] = chunks planned. */
int caddy_debug_gt_scratch_check(caddy_ctx* ctx, int trec, long* out);
long caddy_debug_s16_grad_count(caddy_ctx* ctx);
int caddy_debug_set_pack_merged(caddy_ctx* ctx, int on);      /* tests: 0 = one (un)packing launch per layer and form instead of the job-table launch */
int caddy_debug_dims(caddy_ctx* ctx, int i, int* nhwc4);
int caddy_debug_get(caddy_ctx* ctx, int i, int grad, float* dst_nchw);

/* --- BatchNorm bookkeeping: number of train-mode calls of BN layer `i` since creation (num_batches_tracked) --- */
int caddy_bn_layer_count(caddy_ctx* ctx);
long caddy_bn_calls(caddy_ctx* ctx, int i, char* name_out128);

/* --- per-kernel entry points (unit-parity tests); argument structs are declared in csrc/common.h, pack.h --- */
struct ConvArgs; struct WgradArgs; struct PackDesc; struct TV;
int caddy_k_conv_fwd(const struct ConvArgs* a, void* stream);
int caddy_k_conv_wgrad(const struct WgradArgs* a, void* stream);
/* kernels of the FID feature network (csrc/fid.h; reference: the Conv2d / BatchNorm2d / pooling / F.interpolate calls of torchvision's Inception3 as patched by
 * pytorch_fid/inception.py:143-150,205-322) */
struct IgemmArgs;
size_t caddy_k_igemm_weight_bytes(int Cin, int Cout, int KH, int KW);
int caddy_k_igemm_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KH, int KW,
                       void* w32, void* w16, float* bias_out, void* stream);
int caddy_k_conv_igemm(const struct IgemmArgs* a, void* stream);
int caddy_k_fid_pool(const struct TV* in, const struct TV* out, int mode, void* stream);      /* 0: MaxPool2d(3, 2); 1: avg_pool2d(3, 1, 1, count_include_pad=False); 2: max_pool2d(3, 1, 1); 3: avg_pool2d(3, 1, 1) */
int caddy_k_fid_global_avg(const struct TV* in, double* out, void* stream);
int caddy_k_fid_stage(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, void* stream);
/* the Inception Score's variants (evaluation/metrics/inception_score.py:22,41-43): caddy_k_fid_pool's mode 3 is torchvision's F.avg_pool2d(x, 3, 1, 1) (count_include_pad=True);
 * caddy_k_is_stage is caddy_k_fid_stage without the 2 x - 1; caddy_k_is_softmax: softmax over the C columns of n rows of pitch ld_in -> ld_out floats, one wave64 per row */
int caddy_k_is_stage(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, void* stream);                      /* evaluation/metrics/inception_score.py:22,41 */
int caddy_k_is_softmax(const float* logits, float* probs, int n, int C, long ld_in, long ld_out, void* stream);               /* evaluation/metrics/inception_score.py:43 */
/* kernels of the FVD feature network (csrc/fvd.h; reference: the conv3d / batch norm / max_pool3d ops of the I3D graph behind evaluation/metrics/fvd.py:67-71 and the
 * tf.image.resize_bilinear of fvd.py:52) */
struct Conv3dArgs; struct V5;
size_t caddy_k_conv3d_weight_bytes(int Cin, int Cout, int KT, int KH, int KW);
int caddy_k_conv3d_pack(const float* w_dhwio, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KT, int KH,
                        int KW, void* w32, void* w16, float* bias_out, void* stream);
int caddy_k_conv3d_igemm(const struct Conv3dArgs* a, void* stream);
int caddy_k_fvd_pool(const struct V5* in, const struct V5* out, int kt, int kh, int kw, int st, int sh, int sw, void* stream);      /* max pool, TF SAME padding */
int caddy_k_fvd_stage(const float* src, long frames, int Hs, int Ws, float* out, int Ho, int Wo, void* stream);
int caddy_k_conv_took_direct(void);      /* 1: this thread's last caddy_k_conv_fwd ran on the latency kernel (ConvArgs.direct_ok; model/main_model/model.py:570-607 batch-1 roll-out layers) */
/* BatchNorm fused with the convolutions around it (reference: the conv -> BatchNorm2d -> LeakyReLU chains of model/layers/residual_block.py:51-68,
 * same_block.py:34-47, up_block.py:31-45): per-tile partial sums from the producing conv's epilogue (ConvArgs.stats) -> finalisation without a pass over
 * the tensor; backward of a BatchNorm whose output was never materialised (ConvSrc.bn_scale / bn_shift applied by the consumer while staging) */
int caddy_k_conv_stats_tiles(void);
int caddy_k_bn_finalize_tiles(const float* part, int ntiles, int ldp, long count, const float* gamma, const float* beta, float* rmean, float* rvar, int C,
                              float* mean, float* invstd, float* scale, float* shift, void* stream);
int caddy_k_bn_bwd_lazy(const struct TV* dout, const struct TV* x, const float* mean, const float* invstd, const float* gamma, const float* scale, const float* shift, int act,
                        double* sums, double* scratch, const struct TV* dx, float* dgamma, float* dbeta, void* stream);
int caddy_k_conv_pick_bn(int cout);
/* split 16-bit operand form of a layer's weights for the 16-bit-MFMA convolution (conv_hx.hip): seg < 0 forward, else dgrad of that segment */
int caddy_k_hx_pick_bn(int cout);
int caddy_k_hx_force_big(int v);      /* tests: 1 / 0 force / forbid the 8-wave 16x16x128 tile variant, -1 automatic */
int caddy_k_conv_took_coresident(void);      /* 1: this thread's last split-operand 3x3 launch ran on the co-resident instance of the 16x16x128 tile */
int caddy_k_vgg_beside(int v);        /* co-resident instance of that tile, a mask: bit 0 the VGG19 launches beside the forward pass, bit 1 those beside the BPTT replay, bit 2 every launch on the tile (tests); -1 = CADDY_VGG_BESIDE (default 1) */
int caddy_k_hx_set_bg(int mask);   /* tests / A-B runs: which under-filled k_conv_hx tile variants read their weight fragments straight from global memory (conv_hx.hip, template
                                    * parameter BG; bit 0: 4x16x64, bit 1: 8x16x64, bit 2: 8x16x32 tiles; bit 3: also for workgroups that walk fewer than four 32-channel chunks); -1: the
                                    * CADDY_HX_BG environment variable, default 7 */
long caddy_k_hx_weight_bytes(const struct PackDesc* d, int seg, int rows_pad, int planes);
int caddy_k_pack_hx(const struct PackDesc* d, void* wq, int rows_pad, int seg, int precision, void* stream);
int caddy_k_pack_fwd(const struct PackDesc* d, float* wp, void* stream);
int caddy_k_pack_dgrad(const struct PackDesc* d, int seg, float* wpd, int Cd_pad, int Kd, void* stream);
int caddy_k_unpack_wgrad(const struct PackDesc* d, const float* dwp, void* stream);
int caddy_k_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step, float gscale, void* stream);
/* (pointwise kernels: caddy_k_copy, caddy_k_pool2[_bwd], caddy_k_up2[_bwd], caddy_k_stats, caddy_k_bn_finalize, caddy_k_bn_stats_finalize, caddy_k_bn_apply,
 *  caddy_k_bn_bwd_reduce, caddy_k_bn_bwd_apply, caddy_k_act_bwd_add, caddy_k_lstm_fwd, caddy_k_lstm_bwd, caddy_k_tanh_bwd,
 *  caddy_k_attn_mul[_bwd], caddy_k_gap[_bwd], caddy_k_colsum, caddy_k_spatial_sum, caddy_k_nchw_to_nhwc, caddy_k_nhwc_to_nchw,
 *  caddy_k_batch_sum -- see csrc/capi_kernels.cpp for the exact signatures) */
/* action-network tail, sampling, centroid EMA, their backward, and the loss kernels (csrc/head.h declares the argument structs; reference: model/main_model/action_network.py:86-118,
 * gumbel_softmax.py:25-72, centroid_estimator.py:38-94, training/losses.py, training/trainer.py:447-500).  Every hook and `lv` may be null. */
struct HeadBufs; struct HeadParams; struct SampleCfg; struct SamplerHooks; struct SmallLossArgs; struct DiagArgs; struct LossWeights; struct VggLevels;
int caddy_k_struct_size(int which);      /* sizeof of 0 HeadParams, 1 HeadBufs, 2 SampleCfg, 3 SmallLossArgs, 4 DiagArgs, 5 LossWeights, 6 VggLevels, 7 TV, 8 LpipsLevels, 9 VggCosArgs (ctypes mirrors check themselves); else -1 */
int caddy_k_head_forward(const struct HeadBufs* h, const struct HeadParams* p, int B, int T, void* stream);
int caddy_k_head_sample(const struct HeadBufs* h, const struct HeadParams* p, const struct SampleCfg* c, int NS, float* cen_sums, void (*hook)(float* device_ptr, int count, void* user),
                        void* user, const struct SamplerHooks* sh, void* stream);      /* -1 for K > 16, Da > 8 or K + Da > 16 */
int caddy_k_head_backward(const struct HeadBufs* h, const struct HeadParams* p, const struct SampleCfg* c, int B, int T, int first_call, void* stream);
int caddy_k_head_softmax(const float* logits, float* prob, float* logp /* nullable */, int NS, int K, void* stream);
int caddy_k_loss_l1(const struct TV* gt, const struct TV* rec, const struct TV* drec, int f, int t_off, int Tobs, int Trec, float gscale, double* acc, float* gt_out /* nullable */, void* stream);
int caddy_k_loss_mse(const struct TV* a, const struct TV* b, const struct TV* db, float gscale, double* acc, void* stream);
int caddy_k_loss_small(const struct SmallLossArgs* a, void (*hook)(float* device_ptr, int count, void* user), void* user, void* stream);
int caddy_k_loss_finalize(double* acc, const struct LossWeights* w, double n0, double n1, double n2, double nstates, double nhidden, const struct VggLevels* lv, void* stream);
int caddy_k_loss_diagnostics(const struct DiagArgs* d, const struct TV* states, const struct TV* hidden, void* stream);
int caddy_k_loss_diff_per_frame(const struct TV* a, int Ta, int a_off, const struct TV* b, int Tb, int C, int sq, double* acc, void* stream);
int caddy_k_loss_report_flag(unsigned* flags /* [live n | sticky n] */, int n, double* slot, double* total, void* stream);
/* point-wise and reduction kernels around the VGG trunks (csrc/perceptual.hip, csrc/lpips.hip; csrc/perceptual.h and lpips.h declare the argument structs), launched through the
 * drivers' own format dispatch.  Maps are dense NHWC (pitch == C); *_s16 != 0: that operand is an S16 tensor (csrc/common.h: f16 halves for feature maps, bf16 for gradients).
 * Every entry point validates its arguments first and returns -1 WITHOUT launching for a null pointer, a non-positive size, C % 4 != 0, an S16 operand with C % 32 != 0, a head
 * width outside {64, 128, 256, 512}, f outside {1, 2, 4} or an observation that is not f times the output, a time window that leaves the sequence, a partial slab too small. */
struct VggCosArgs; struct LpipsLevels;
int caddy_k_vgg_maxpool2(const float* in, float* out, int N, int H, int W, int C, void* stream);      /* MaxPool2d(2, 2), fp32; out (N, H / 2, W / 2, C) */
int caddy_k_vgg_maxpool2_bwd_relu(const float* a, int a_s16, const float* gp, float* gz, int gz_s16, int N, int H, int W, int C, void* stream);      /* gz (N, H, W, C) assigned: gradient of max_pool2d(relu(a), 2) */
int caddy_k_vgg_feat_l1(const float* rec, int rec_s16, const float* gt, int gt_s16, int N, int H, int W, int C, float seed_w, float* gz /* nullable */, int gz_s16, double* acc,
                        void* stream);      /* acc[0] += sum |rec - gt|; gz = seed_w sign(rec - gt) where rec > 0, else 0 */
int caddy_k_vgg_feat_l1_img(const float* rec, int rec_s16, const float* gt, int gt_s16, int N, int H, int W, int C, double* acc, void* stream);      /* acc[n] += image n's sum */
int caddy_k_vgg_cos_blocks(int H, int W, int C);      /* partial triples per image and level that caddy_k_vgg_feat_cos writes */
int caddy_k_vgg_feat_cos(const struct VggCosArgs* a, int nf, double* part, long part_doubles, double* out, void* stream);      /* out[n] = mean over the five levels of the cosine similarity */
int caddy_k_vgg_metric_stage(const float* src, float* out, int N, int H, int W, float range, void* stream);      /* (N, 3, H, W) in [0, range] -> (N, H, W, 4) */
int caddy_k_vgg_gt_resize(const struct TV* obs, float* out, int Ho, int Wo, int B, int Tobs, int Trec, int t_off, int f, void* stream);      /* out (B * Trec, Ho, Wo, 4) */
int caddy_k_vgg_time_chunk(float* full, float* chunk, int B, int Tfull, long F4, int t0, int len, int add, void* stream);
int caddy_k_vgg_copy_f(const float* src, float* dst, long n, void* stream);
int caddy_k_lpips_blocks(int npix);      /* partials per frame of a level with npix pixels */
int caddy_k_lpips_stage(const float* src, float* out, int N, int H, int W, float range, void* stream);
int caddy_k_lpips_head(const float* f0, int s0, const float* f1, int s1, const float* w, int nf, int npix, int C, int blocks, double* part /* [n * blocks + b] */, void* stream);
int caddy_k_lpips_finalize(const double* part, const struct LpipsLevels* lv, long part_doubles, int nf, double* out /* (6, ldo) */, int ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif
