/*
 * eamm_hip.h -- C ABI of libeamm_hip.so: the MI355X (gfx950) implementation of EAMM's
 * dense-motion + OcclusionAwareGenerator forward path, the key-point detectors, the audio
 * deconvolution tail and the emotion detector Emotion_k that feed it.
 *
 * The reference has no FFI layer for this path: its boundary is the Python nn.Module
 * `OcclusionAwareGenerator` (reference modules/generator.py:8-97).  The entry points below are what
 * a binding for that module needs (see INTEGRATION.md for the ctypes stub); every one cites the
 * reference interface it stands in for.
 *
 * Conventions
 *   - every function returns 0 on success, a negative eamm_status otherwise; the message is
 *     available from eamm_last_error(ctx) (ctx may be NULL for a failed eamm_create);
 *   - the CALLER owns every device buffer passed in or out; the library owns only its handle, the
 *     packed weights, the cached source tensors and its workspace;
 *   - all work is enqueued on the caller's stream (a hipStream_t passed as void*); no call
 *     synchronises the device except eamm_create / eamm_finalize_weights / eamm_destroy;
 *   - one handle per (device, stream); handles are independent, so different host threads may
 *     drive different handles concurrently (reference threading model: one module replica per
 *     device, train.py:53-63);
 *   - boundary tensors are float32, contiguous, NCHW -- the reference's layout -- unless stated.
 */
#ifndef EAMM_HIP_H_
#define EAMM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAMM_ABI_VERSION 6

typedef enum eamm_status {
    EAMM_OK = 0,
    EAMM_ERR_ARG = -1,        /* bad argument / unsupported configuration            */
    EAMM_ERR_STATE = -2,      /* call order (weights not finalised, no source cached) */
    EAMM_ERR_KEY = -3,        /* unknown / missing / mis-shaped state_dict entry      */
    EAMM_ERR_HIP = -4,        /* HIP runtime error                                    */
    EAMM_ERR_NUMERIC = -5     /* singular key-point jacobian                          */
} eamm_status;

typedef struct eamm_ctx eamm_ctx;

/*
 * Constructor arguments of OcclusionAwareGenerator (reference modules/generator.py:14-15) with
 * dense_motion_params (reference modules/dense_motion.py:12-13) flattened in, plus the two sizes
 * the workspace is allocated for.  Any positive channel widths: those that are not multiples of the kernels' 32-channel
 * granule are served by padding the state_dict at eamm_finalize_weights (the extra channels carry exact zeros); a
 * training-mode handle (eamm_set_training) needs multiples of 32 and three image channels.  num_channels: 1 .. 6 -- one
 * or two channels run as the equivalent three-channel network (zero filters on the channels that do not exist); four to six
 * (RGBA ...) run as TWO groups of three channels through the motion kernels (a pixel's image channels live in one float4
 * beside its heat-map value per group: motion.hip) with `final` on the generic 7x7 kernel; sources and outputs keep the
 * reference's shapes [.,C,H,W] throughout; seven and more are refused.
 */
typedef struct eamm_config {
    int32_t num_channels;            /* 3 (1 .. 6 accepted)                            */
    int32_t num_kp;                  /* 10                                             */
    int32_t block_expansion;         /* 64                                             */
    int32_t max_features;            /* 512                                            */
    int32_t num_down_blocks;         /* 2                                              */
    int32_t num_bottleneck_blocks;   /* 6                                              */
    int32_t estimate_occlusion_map;  /* 0 / 1                                          */
    int32_t dm_block_expansion;      /* dense_motion_params.block_expansion            */
    int32_t dm_max_features;         /* dense_motion_params.max_features               */
    int32_t dm_num_blocks;           /* dense_motion_params.num_blocks                 */
    int32_t dm_inv_scale;            /* 1 / dense_motion_params.scale_factor (1, 2, 4) */
    float   kp_variance;             /* dense_motion_params.kp_variance, default 0.01  */
    int32_t height, width;           /* frame size (multiple of 2^max(down, log2 inv_scale + dm_num_blocks)) */
    int32_t max_frames;              /* frames per eamm_forward_frames call the workspace holds */
    int32_t max_sources;             /* source images cached at once (1 for a clip)    */
} eamm_config;

/* Optional outputs of a forward call; NULL pointers are skipped.  Shapes for n frames, frame
 * HxW, motion grid hxw = H/inv_scale x W/inv_scale, K = num_kp (reference generator.py:70-95). */
typedef struct eamm_outputs {
    float* prediction;       /* [n,C,H,W]      'prediction'      -- required (C = num_channels) */
    float* mask;             /* [n,K+1,h,w]    'mask'                                   */
    float* sparse_deformed;  /* [n,K+1,C,h,w]  'sparse_deformed'                        */
    float* occlusion_map;    /* [n,1,h,w]      'occlusion_map'                          */
    float* deformed;         /* [n,C,H,W]      'deformed'                               */
    float* deformation;      /* [n,h,w,2]      dense_motion 'deformation' (internal to the reference) */
    uint8_t* frames_u8;      /* [n,H,W,3] uint8 = round(255*prediction), HWC: the layout demo.py:281,507 saves (C = 3 only) */
} eamm_outputs;

int eamm_abi_version(void);

/* Replaces OcclusionAwareGenerator.__init__ (generator.py:14-48) + .cuda() (demo.py:56-57). */
int eamm_create(const eamm_config* cfg, int device, eamm_ctx** out);
void eamm_destroy(eamm_ctx* ctx);
const char* eamm_last_error(const eamm_ctx* ctx);

/*
 * Replaces generator.load_state_dict(checkpoint['generator']) (demo.py:91, logger.py:58): call
 * once per state_dict entry with the reference's key (e.g. "bottleneck.r0.conv1.weight") and a
 * HOST float32 pointer (num_batches_tracked entries may be skipped), then eamm_finalize_weights,
 * which checks the key set strictly, folds eval-mode BatchNorm (sync_batchnorm/batchnorm.py:48-53)
 * into the adjacent convolutions and repacks OIHW weights into MFMA tile order on the device.
 */
int eamm_load_tensor(eamm_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int eamm_finalize_weights(eamm_ctx* ctx);

/*
 * Frame-invariant part of OcclusionAwareGenerator.forward, hoisted out of the per-frame loop
 * (generator.py:61-63 encoder, dense_motion.py:83 anti-alias down-sampling): caches, for `ns`
 * source images [ns,C,H,W] on the device, the encoder feature map, the down-sampled source and the
 * full-resolution source.
 */
int eamm_encode_source(eamm_ctx* ctx, const float* source, int ns, void* stream);

/*
 * Per-frame part of OcclusionAwareGenerator.forward (generator.py:68-95, dense_motion.py:81-113)
 * for n driving key-point sets.  kp_*_value: [*,K,2]; kp_*_jacobian: [*,K,2,2] or NULL (both or
 * neither; NULL = the "'jacobian' not in kp_driving" branch, dense_motion.py:55).  kp_source_* hold
 * `ns` sets matching the cached sources; ns == 1 broadcasts one source to all frames (the clip
 * loop, demo.py:251-281), otherwise ns == n and frame i uses source i (the module's batch contract).
 */
int eamm_forward_frames(eamm_ctx* ctx, int n,
                        const float* kp_driving_value, const float* kp_driving_jacobian,
                        const float* kp_source_value, const float* kp_source_jacobian,
                        const eamm_outputs* outputs, void* stream);

/*
 * torch.inverse raises on a singular key-point jacobian (dense_motion.py:56) and synchronises to do
 * so.  The kernels only record the condition; this call synchronises `stream` and returns
 * EAMM_ERR_NUMERIC if any forward call since the last check met one (outputs are then inf/nan).
 */
int eamm_check_numeric(eamm_ctx* ctx, void* stream);

/*
 * Cached source tensors as one flat device blob, so that a clip's source can be encoded on one
 * GPU and broadcast to the others (RCCL) instead of re-encoded: export copies the cache of the
 * `ns` encoded sources into `dst`, import installs such a blob.  Both are stream-ordered copies.
 */
size_t eamm_source_cache_bytes(const eamm_ctx* ctx, int ns);
int eamm_export_source_cache(eamm_ctx* ctx, void* dst, int ns, void* stream);
int eamm_import_source_cache(eamm_ctx* ctx, const void* src, int ns, void* stream);

/* Algorithmic work of one eamm_forward_frames call of n frames (for roofline accounting). */
double eamm_flops_per_frame(const eamm_ctx* ctx);
double eamm_encode_flops(const eamm_ctx* ctx);
/* Form the bottleneck ResBlock2d convolutions take for a call of n frames: 0 = direct, 2 = Winograd F(2x2,3x3),
 * 4 = Winograd F(4x4,3x3) (executed multiplies = 1, 4/9, 1/4 of the reference's; negative on a bad handle). */
int eamm_bottleneck_form(const eamm_ctx* ctx, int n);
/* Chains the bottleneck of a call of n frames is split into (1 = one launch sequence on the caller's stream; K > 1 =
 * K groups of whole frames on K streams forked from and joined back into the caller's stream inside the call). */
int eamm_bottleneck_chains(const eamm_ctx* ctx, int n);
/* Of those, the chains that cover the WHOLE per-frame pass (independent launch sequences whose bottleneck launches
 * time-share the chip) rather than the bottleneck alone: 1 = none. */
int eamm_pass_chains(const eamm_ctx* ctx, int n);
/* Which side streams the last eamm_forward_frames call ran its chains on: 0 = the device's shared pool, 1 = the handle's private
 * streams because another host thread held the pool, 2 = private because the caller's stream was being captured into a graph
 * (side streams join the capture until it ends, so a captured call never touches the shared pool). */
int eamm_last_stream_set(const eamm_ctx* ctx);
/* The launch plan of a call of n frames as a JSON object (chains, frames per chain, bottleneck form, hourglass level forms,
 * final-layer kernel ...), written NUL-terminated into buf[cap]; returns the length needed.  For benchmark records. */
int eamm_describe_plan(const eamm_ctx* ctx, int n, char* buf, int cap);
/* Every EAMM_* knob the library has read so far in this process, as a JSON object {"NAME": {"value": v, "set": 0|1|2}}
 * (value in effect; set = 1: the environment supplied it; 2: present in the environment but IGNORED).  Same buffer contract as
 * eamm_describe_plan.
 * DOCUMENTED knobs -- selectors of a computation form or of the launch plan; every setting computes the same frames up to rounding:
 *   EAMM_PASS_CHAINS / EAMM_BNECK_CHAINS   chains of a call over the whole pass / inside the bottleneck (0 = automatic, 1 = off)
 *   EAMM_WINO_TILE (4 | 2), EAMM_WINO_MIN_M (< 0: direct), EAMM_WINO4_MIN_M    bottleneck form: F(4x4), F(2x2), direct
 *   EAMM_ENC_WINO, EAMM_PATCH_POLY, EAMM_HEAD_ROWSPLIT, EAMM_COL7, EAMM_FIRST7, EAMM_FINAL_FUSED, EAMM_KPA_THIN
 *                                          (0 | 1) the alternative kernel of a stage: hourglass encoder, up blocks, flow head, 7x7 layers,
 *                                          KPDetector_a's heads (wide + thin split | one padded convolution)
 *   EAMM_WGRAD_WINO4, EAMM_WGRAD_ROW, EAMM_CONV_DEV_WINO4   (0 | 1) forms of the training operators
 *   EAMM_PRIVATE_STREAMS (0 | 1)           never use the shared side-stream pool
 *   EAMM_WINO4_VARIANT (0 | 3 | 6)         software pipeline of the F(4x4) bottleneck GEMM, pinned for every call size; unset: 6 (variant 3 with
 *                                          the transformed input loaded non-temporally) while the call's GEMM workgroups number at most the CUs,
 *                                          3 above (bit-identical results); eamm_create refuses any other value
 * TUNING aids (tile-size thresholds, pipeline variants, split sizes: everything else the sources read) are honoured only together
 * with EAMM_TUNING=1; without it they are ignored and reported with "set": 2.
 * Knobs that compute WRONG results (timing experiments: EAMM_WINO4_EPI_V, EAMM_COL7_DBG, EAMM_WINO4_VARIANT 10/16/17/50) exist
 * only in a build with -DEAMM_EXPERIMENTS (make EXPERIMENTS=1); the product library's eamm_create fails when one of them is set.
 * EAMM_WARP_JOINT (a scheduling variant measured in round 4, -0.8 % frames/s) has been removed: eamm_create fails when it is set
 * to non-zero. */
int eamm_knobs_json(char* buf, int cap);
/* Executed matrix-core flops (what the launched grids really issue: padded tiles, Winograd / polyphase point counts -- not the
 * reference convolution's) of every kernel enqueued through the library in this PROCESS so far, all host threads (autograd runs
 * the backward operators on its own thread): a monotonic total; difference two readings around a step (bench.py
 * `train_step.roofline`).  eamm_forward_frames keeps its own per-call count for the profile keys. */
double eamm_total_mfma_flops(void);
/* 1 when this library was built with -DEAMM_EXPERIMENTS (never benchmark or ship such a build), else 0. */
int eamm_build_experiments(void);

/*
 * ---- key-point detectors -----------------------------------------------
 * Constructor arguments of KPDetector / KPDetector_a (reference modules/keypoint_detector.py:12-14, 115-117).
 * with_predictor = 1: KPDetector -- eamm_kp_detect(image) runs anti-alias down-sampling, the `predictor`
 * hourglass and the heads (keypoint_detector.py:77-105; once per clip on the source, demo.py:206).
 * with_predictor = 0: KPDetector_a -- eamm_kp_detect_features(feature_map) runs only the heads on a caller-
 * provided [B, block_expansion + in_features, H/inv_scale, W/inv_scale] map (keypoint_detector.py:180-205;
 * once per frame, demo.py:219); `predictor.*` / `down.weight` entries need not be loaded for it.
 */
typedef struct eamm_kp_ctx eamm_kp_ctx;
typedef struct eamm_kp_config {
    int32_t num_kp;                 /* 10                                                   */
    int32_t num_channels;           /* 3 (1 .. 8 accepted)                                   */
    int32_t in_features;            /* hourglass input channels: num_channels (KPDetector) or num_channels_a */
    int32_t block_expansion;        /* 32                                                   */
    int32_t max_features;           /* 1024                                                 */
    int32_t num_blocks;             /* 5                                                    */
    float   temperature;            /* 0.1                                                  */
    int32_t estimate_jacobian;      /* 0 / 1                                                */
    int32_t single_jacobian_map;    /* 0 / 1                                                */
    int32_t inv_scale;              /* 1 / scale_factor (1, 2, 4)                           */
    int32_t pad;                    /* padding of the 7x7 heads: 0 (reference default) or 3 */
    int32_t height, width;          /* image size; feature maps are height/inv_scale x width/inv_scale */
    int32_t max_batch;
    int32_t with_predictor;
} eamm_kp_config;

typedef struct eamm_kp_outputs {    /* 'value' required; NULL pointers are skipped           */
    float* value;                   /* [B,K,2]     soft-argmax key points, (x, y) in [-1,1] */
    float* jacobian;                /* [B,K,2,2]                                            */
    float* heatmap;                 /* [B,K,h-6+2*pad,w-6+2*pad]                            */
} eamm_kp_outputs;

int eamm_kp_create(const eamm_kp_config* cfg, int device, eamm_kp_ctx** out);
void eamm_kp_destroy(eamm_kp_ctx* ctx);
const char* eamm_kp_last_error(const eamm_kp_ctx* ctx);
int eamm_kp_load_tensor(eamm_kp_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int eamm_kp_finalize_weights(eamm_kp_ctx* ctx);
int eamm_kp_detect(eamm_kp_ctx* ctx, const float* image /*[B,3,H,W]*/, int B, const eamm_kp_outputs* out, void* stream);
int eamm_kp_detect_features(eamm_kp_ctx* ctx, const float* feature_map, int B, const eamm_kp_outputs* out, void* stream);
/* Round 6 -- the private hand-over between the deconvolution tail and KPDetector_a (reference: util.py:604-607 produces
 * deco_out[:, t], keypoint_detector.py:180-205 consumes it; both sides live in this library, so the [B,35,64,64] NCHW tensor the
 * reference materialises between them is optional).  eamm_kp_split_channels: the `wide` channel count 32 m this handle's heads
 * read (feature map = 32 m + 3 channels, heads in the wide + thin form), or 0.  eamm_kp_detect_features_split: `wide` NHWC
 * [B,h,w,32 m] float32 + `thin` [B,h,w,4] (the last three channels and a zero), both caller-owned device memory, as written by
 * eamm_deconv_forward_split; same outputs as eamm_kp_detect_features on the equivalent NCHW map, bit for bit. */
int eamm_kp_split_channels(const eamm_kp_ctx* ctx);
int eamm_kp_detect_features_split(eamm_kp_ctx* ctx, const float* wide, const float* thin, int B, const eamm_kp_outputs* out, void* stream);

/*
 * ---- emotion detector Emotion_k (reference modules/util.py:1223-1527, demo.py:68-70, --type linear_3) ------------------
 * eamm_emo_detect runs Emotion_k.forward (util.py:1498-1527) and Emotion_k.feature (:1477-1496) in eval mode in ONE pass
 * (demo.py:221-228 calls both per frame; the trunk is computed once here): anti-alias down-sampling + the `predictor` hourglass
 * (the key-point detector's, hourglass_common.h), the 3x3 stem + BatchNorm + ReLU + MaxPool2d(3,2,1), the ResNet-18 trunk
 * (layer1..layer4 of BasicBlocks; stride-2 3x3 and 1x1 convolutions in conv_s2.hip), AdaptiveAvgPool2d(1), and the head:
 * classify.last_fc, the positional embedding get_embedder(10) of (value, jacobian) (accurate sinf / cosf), fc_p, fc_all and
 * the Conv1d `final` stack.  Every BatchNorm folds at finalize.  `fc`, `fc_n`, `final_4`, `final_10` are accepted by
 * eamm_emo_load_tensor and ignored (unused by forward).  The head hard-codes 10 input key points (fc_p: 10 x 126 inputs).
 */
typedef struct eamm_emo_ctx eamm_emo_ctx;
typedef struct eamm_emo_config {
    int32_t block_expansion;        /* 32                                                           */
    int32_t num_channels;           /* 3 (1 .. 8 accepted)                                          */
    int32_t max_features;           /* 1024                                                         */
    int32_t num_blocks;             /* 5                                                            */
    int32_t inv_scale;              /* 1 / scale_factor (1, 2, 4); the demo's 0.25 -> 4             */
    int32_t num_classes;            /* outputs of classify.last_fc (8 in the reference)             */
    int32_t height, width;          /* image size                                                   */
    int32_t max_batch;
} eamm_emo_config;

typedef struct eamm_emo_outputs {   /* caller-owned device buffers; NULL pointers are skipped        */
    float* value;                   /* [B,4,2]            kp['value']                               */
    float* jacobian;                /* [B,4,2,2]          kp['jacobian']                            */
    float* fake;                    /* [B,num_classes]    classify(out)                             */
    float* feature;                 /* [B,512]            Emotion_k.feature(x): the pooled trunk    */
} eamm_emo_outputs;

int eamm_emo_create(const eamm_emo_config* cfg, int device, eamm_emo_ctx** out);
void eamm_emo_destroy(eamm_emo_ctx* ctx);
const char* eamm_emo_last_error(const eamm_emo_ctx* ctx);
int eamm_emo_load_tensor(eamm_emo_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int eamm_emo_finalize_weights(eamm_emo_ctx* ctx);
/* image [B,C,H,W], kp_value [B,10,2], kp_jacobian [B,10,2,2] (both may be NULL when only `feature` / `fake` are asked for) */
int eamm_emo_detect(eamm_emo_ctx* ctx, const float* image, const float* kp_value, const float* kp_jacobian, int B,
                    const eamm_emo_outputs* out, void* stream);

/*
 * ---- audio network AT_net2 up to its LSTM (reference modules/util.py:514-600; demo.py:286-354 test_auido) ------------------
 * eamm_audio_lstm_features computes AT_net2's lstm_out [N,T,256] in eval mode: the image encoder (eight DownBlock2d: conv 3x3 +
 * BatchNorm + ReLU + AvgPool2d(2), 3 -> 512 channels, 256x256 -> 1x1) once per clip; the audio encoder (conv2d blocks with
 * BatchNorm folded, two MaxPool2d(3)), audio_eocder_fc * weight and pose_encoder over every step; then the three-layer
 * nn.LSTM(1024, 256) from the zero state or a given one.  Steps run max_batch / N at a time (encoders, input projections, then
 * the recurrence of each layer as one persistent launch); results do not depend on how a clip is split into calls: a clip
 * computed in chunks with the state carried (h_out / c_out of one call as h0 / c0 of the next) is bit-identical to one call.
 * State-dict keys: the reference's 235 except decon.* (DeconvTail's handle) and generator.* (unused StyleGAN2 branch).  Calls on
 * one handle must be issued to one stream at a time.  A recurrence that cannot complete (a workgroup waiting longer than the
 * wall-clock limit for another) sets a sticky error word: eamm_audio_check (after synchronising `stream`, when given) and every
 * later call on the handle then fail with EAMM_ERR_HIP.
 */
typedef struct eamm_audio_ctx eamm_audio_ctx;
typedef struct eamm_audio_config {
    int32_t max_batch;              /* steps x clips per encoder pass (8 .. 4096)                      */
    int32_t reserved[3];
} eamm_audio_config;

int eamm_audio_create(const eamm_audio_config* cfg, int device, eamm_audio_ctx** out);
void eamm_audio_destroy(eamm_audio_ctx* ctx);
const char* eamm_audio_last_error(const eamm_audio_ctx* ctx);
int eamm_audio_load_tensor(eamm_audio_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int eamm_audio_finalize_weights(eamm_audio_ctx* ctx);
/* image [N,3,256,256], audio [N,T,28,12], pose [N,T,6], out [N,T,256]: device fp32, 1 <= N <= 8, T >= 1.  h0 / c0: [3,N,256]
 * (layer-major, as nn.LSTM's hidden tuple) or NULL for zeros; h_out / c_out: [3,N,256] or NULL (may be h0 / c0 themselves).
 * clip_bias: NULL or [N,1024], the image's share of the layer-0 gates (W_ih_l0[:, :512] image_feature + both layer-0 biases):
 * written when `image` is given; with image NULL it is read instead, so the later chunks of a clip skip the image encoder. */
int eamm_audio_lstm_features(eamm_audio_ctx* ctx, const float* image, const float* audio, const float* pose, int N, int T, float weight,
                             const float* h0, const float* c0, float* h_out, float* c_out, float* clip_bias, float* out, void* stream);
/* EAMM_OK, or EAMM_ERR_HIP once a recurrence has timed out; stream non-NULL: synchronised first, so the calls issued to it are covered */
int eamm_audio_check(eamm_audio_ctx* ctx, void* stream);

/*
 * ---- N3: audio-to-feature deconvolution tail ------------------------------------------------------------
 * Replaces the nn.Sequential `AT_net2.decon` (reference modules/util.py:559-576), which the reference evaluates
 * once per frame on the LSTM output (util.py:604-607) to produce the [35,64,64] maps KPDetector_a consumes
 * (demo.py:219): num_layers ConvTranspose2d layers -- the first 6x6 / stride 2 / padding 1 on the 1x1 input, the
 * rest 4x4 / stride 2 / padding 1 -- each but the last followed by eval-mode BatchNorm2d + ReLU.
 * State-dict keys are the Sequential's: "0.weight" [C0,C1,6,6], "0.bias", "1.weight", "1.bias", "1.running_mean",
 * "1.running_var", "3.weight" [C1,C2,4,4], ... (strict check in eamm_deconv_finalize_weights).
 */
typedef struct eamm_deconv_ctx eamm_deconv_ctx;

typedef struct eamm_deconv_config {
    int32_t num_layers;     /* reference: 5                                                          */
    int32_t channels[9];    /* [0] input features (256); [i+1] outputs of layer i (256,128,128,128,35);
                             * every layer INPUT width must be a multiple of 32                      */
    int32_t max_batch;      /* frames per eamm_deconv_forward call                                   */
} eamm_deconv_config;

int eamm_deconv_create(const eamm_deconv_config* cfg, int device, eamm_deconv_ctx** out);
void eamm_deconv_destroy(eamm_deconv_ctx* ctx);
const char* eamm_deconv_last_error(const eamm_deconv_ctx* ctx);
int eamm_deconv_load_tensor(eamm_deconv_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int eamm_deconv_finalize_weights(eamm_deconv_ctx* ctx);
/* x: [B, channels[0]] (= the reference's [B,C,1,1]) device fp32; out: [B, channels[L], S, S] NCHW, S = 4 << (L-1). */
int eamm_deconv_forward(eamm_deconv_ctx* ctx, const float* x, int B, float* out, void* stream);
/* Round 6: the same layers with the last one writing the split NHWC form KPDetector_a's heads read (above) instead of NCHW:
 * wide [B,S,S,C_last - 3], thin [B,S,S,4].  eamm_deconv_split_channels: C_last - 3 when that is a positive multiple of 32, else 0
 * (eamm_deconv_forward_split then fails with EAMM_ERR_ARG). */
int eamm_deconv_split_channels(const eamm_deconv_ctx* ctx);
int eamm_deconv_forward_split(eamm_deconv_ctx* ctx, const float* x, int B, float* wide, float* thin, void* stream);

/*
 * ---- N4: training-mode BatchNorm, forward (round 2) and backward (round 3) --------------------------------------
 * Replaces the arithmetic of _SynchronizedBatchNorm.forward (reference sync_batchnorm/batchnorm.py:46-125) on NCHW
 * float32 device tensors; the reduction over replicas (ReduceAddCoalesced / Broadcast, batchnorm.py:102-105) is the
 * caller's all-reduce of `sums` between eamm_bn_local_sums and eamm_bn_finalize (torch.distributed / RCCL).
 * Stateless: the caller owns every buffer and makes the tensors' device current; work is enqueued on `stream`.
 *   eamm_bn_local_sums   sums[c] = sum over (N, HW) of x[:, c], sums[C + c] = sum of squares (batchnorm.py:61-64);
 *                        sums[2C] + 4096 * sums[2C+1] = N * HW as two exact floats, so that element counts add up
 *                        through the same float all-reduce -- all-reduce THESE 2C+2 floats.  `sums` holds 6C+2 floats:
 *                        behind the exchanged part sit the same 2C totals in double (8-byte aligned), which
 *                        EAMM_BN_SINGLE uses.  workspace: eamm_bn_workspace_floats(N, C, HW) floats, 8-byte aligned.
 *   eamm_bn_finalize     mean[c], scale[c] = inv_std * weight[c] and the running-statistics update (momentum, unbiased
 *                        variance) of _compute_mean_std (batchnorm.py:110-125).  mode EAMM_BN_SYNC: the replicas' path,
 *                        inv_std = clamp(biased var, eps)^-0.5; EAMM_BN_SINGLE: F.batch_norm(training=True)
 *                        (batchnorm.py:48-53), inv_std = 1/sqrt(biased var + eps); EAMM_BN_EVAL: running statistics,
 *                        nothing updated (sums may be NULL).  weight may be NULL (affine=False).
 *                        inv_std (optional, [C]): the inverse standard deviation alone -- what the backward needs.
 *   eamm_bn_apply        y = (x - mean[c]) * scale[c] + bias[c] (batchnorm.py:74-79); bias may be NULL.
 * Backward (round 3) -- the gradient autograd derives from those lines, with xhat = (x - mean) * inv_std:
 *   eamm_bn_backward_sums      sums[c] = sum dy, sums[C + c] = sum dy * (x - mean[c]) over this replica's shard, packed like
 *                              eamm_bn_local_sums' output (6C+2 floats): all-reduce the first 2C+2 floats INTO A COPY --
 *   eamm_bn_backward_finalize  takes both: dbias = local sum dy, dweight = local sum dy * xhat (this replica's shard; the
 *                              reduction of parameter gradients over replicas is the caller's, as under DistributedDataParallel),
 *                              and coef[3C] = (S1 / N, S2 * inv_std^2 / N, weight * inv_std) from the REDUCED sums (all replicas);
 *                              mode as eamm_bn_finalize (EAMM_BN_EVAL: statistics are constants, S-terms vanish; EAMM_BN_SYNC: a
 *                              channel whose variance was clamped to eps has no gradient through the variance).
 *   eamm_bn_backward_apply     dx = coef_s * (dy - coef_a - (x - mean) * coef_b).
 */
#define EAMM_BN_SYNC 0
#define EAMM_BN_SINGLE 1
#define EAMM_BN_EVAL 2
size_t eamm_bn_workspace_floats(int N, int C, int HW);
int eamm_bn_local_sums(const float* x, int N, int C, int HW, float* sums /*[6C+2]*/, float* workspace, void* stream);
int eamm_bn_finalize(const float* sums, int C, float eps, float momentum, int mode, const float* weight,
                     float* running_mean, float* running_var, float* mean /*[C]*/, float* scale /*[C]*/, float* inv_std /*[C] or NULL*/,
                     void* stream);
int eamm_bn_backward_sums(const float* x, const float* dy, const float* mean, int N, int C, int HW, float* sums /*[6C+2]*/,
                          float* workspace, void* stream);
int eamm_bn_backward_finalize(const float* local_sums, const float* reduced_sums, int C, const float* inv_std, const float* weight,
                              float eps, int mode, float* dweight /*[C] or NULL*/, float* dbias /*[C] or NULL*/, float* coef /*[3C]*/,
                              void* stream);
int eamm_bn_backward_apply(const float* x, const float* dy, const float* mean, const float* coef, int N, int C, int HW, float* dx,
                           void* stream);

/* The same BatchNorm on NHWC activations x [B,H,W,C] (= [M,C], M = B*H*W; what the path's convolutions produce), fused with the
 * tail of the reference's blocks (modules/util.py:858-938): y = [avgpool2x2](act((x - mean) * scale + bias)), relu = 1 | 0,
 * pool = 1 | 0 (DownBlock2d; H, W even; y is [B,H/2,W/2,C]).  Statistics / finalize / backward_finalize are the layout-free
 * entries above (same packed `sums`).  Backward: grad_out has y's shape; the ReLU mask is recomputed from x, so x is all the
 * forward keeps.  C a multiple of 4, at most 1024. */
size_t eamm_bn_nhwc_workspace_floats(long long M, int C);
int eamm_bn_nhwc_local_sums(const float* x, long long M, int C, float* sums, float* workspace, void* stream);
int eamm_bn_nhwc_apply(const float* x, const float* mean, const float* scale, const float* bias, int B, int H, int W, int C, int relu,
                       int pool, float* y, void* stream);
int eamm_bn_nhwc_backward_sums(const float* x, const float* grad_out, const float* mean, const float* scale, const float* bias, int B,
                               int H, int W, int C, int relu, int pool, float* sums, float* workspace, void* stream);
int eamm_bn_nhwc_backward_apply(const float* x, const float* grad_out, const float* mean, const float* scale, const float* bias,
                                const float* coef, int B, int H, int W, int C, int relu, int pool, float* grad_x, void* stream);
/* One replica (nothing to all-reduce between the sums and their finalize step): eamm_bn_nhwc_local_sums + eamm_bn_finalize, and
 * eamm_bn_nhwc_backward_sums + eamm_bn_backward_finalize (reduced_sums == local_sums), each as ONE call -- the finalize step runs
 * in the kernel that adds the slices up, on the values the separate entry would read back (bit-identical results, two launches
 * fewer per BatchNorm site and direction).  mode 0 | 1 as eamm_bn_finalize; `sums` is still written. */
int eamm_bn_nhwc_local_stats(const float* x, long long M, int C, float eps, float momentum, int mode, const float* weight,
                             float* running_mean, float* running_var, float* sums, float* mean, float* scale, float* inv_std,
                             float* workspace, void* stream);
int eamm_bn_nhwc_backward_local(const float* x, const float* grad_out, const float* mean, const float* scale, const float* bias, int B,
                                int H, int W, int C, int relu, int pool, const float* inv_std, const float* weight, float eps, int mode,
                                float* sums, float* grad_weight /*[C] or NULL*/, float* grad_bias /*[C] or NULL*/, float* coef /*[3C]*/,
                                float* workspace, void* stream);
int eamm_bn_apply(const float* x, const float* mean, const float* scale, const float* bias, int N, int C, int HW, float* y,
                  void* stream);
const char* eamm_bn_last_error(void);

/*
 * ---- N4, second slice (round 3): the generator's forward in TRAINING mode ------------------------------------------------
 * Replaces OcclusionAwareGenerator.forward when the module is in .train() (the fine-tuning loop, reference train.py:133):
 * every SynchronizedBatchNorm2d inside SameBlock2d / DownBlock2d / UpBlock2d / ResBlock2d (modules/util.py:858-938) then
 * normalises with the statistics of the batch (sync_batchnorm/batchnorm.py:55-125) and updates its running statistics.
 *   eamm_set_training(ctx, 1)  before eamm_finalize_weights: convolutions are packed with their RAW weights (no BatchNorm
 *                              folded in); eamm_encode_source / eamm_forward_frames of such a handle would run without
 *                              any normalisation and must not be used.
 *   eamm_train_num_sites / eamm_train_site_name   the BatchNorm sites of one forward in execution order, named by their
 *                              state_dict prefix ("first.norm", "bottleneck.r0.norm1", ...).
 *   eamm_train_begin           lays out one forward over n (source, key point) pairs -- source [n,3,H,W]; key points as for
 *                              eamm_forward_frames with one source set per frame -- and the caller's BatchNorm tensors
 *                              (device pointers, one eamm_bn_site per site: running_mean / running_var are UPDATED in place
 *                              with `momentum`, batchnorm.py:110-125).  sync = 0: F.batch_norm's formula (one replica,
 *                              batchnorm.py:48-53), 1: the replicas' formula.  sums_buffer: caller-owned device buffer of
 *                              6 * eamm_train_max_channels(ctx) + 2 floats, 8-byte aligned, that stays valid until the
 *                              last eamm_train_next.  Nothing is enqueued yet.
 *   eamm_train_next            enqueues the forward up to the next BatchNorm's statistics and returns 1 with
 *                              *nfloats = 2C + 2: the first 2C + 2 floats of sums_buffer hold per-channel sum, sum of
 *                              squares and the element count as in eamm_bn_local_sums -- ALL-REDUCE them over the replicas on the
 *                              same stream (nothing to do on one replica) and call again; returns 0 when the outputs given
 *                              to eamm_train_begin are complete (stream-ordered), < 0 on error.
 * Forward only: the outputs carry no gradient (the backward pass is composed from the differentiable operator entries further
 * down -- eamm_op_conv_dev, eamm_op_conv_wgrad, eamm_op_warp_backward, ... -- by eamm_amd/train_graph.py, not by this forward).
 */
typedef struct eamm_bn_site {
    const float* weight;     /* [C] device                                  */
    const float* bias;       /* [C] device                                  */
    float* running_mean;     /* [C] device, updated                         */
    float* running_var;      /* [C] device, updated (unbiased batch variance) */
} eamm_bn_site;
int eamm_set_training(eamm_ctx* ctx, int on);
int eamm_train_num_sites(const eamm_ctx* ctx);
const char* eamm_train_site_name(const eamm_ctx* ctx, int i);
int eamm_train_max_channels(const eamm_ctx* ctx);
int eamm_train_begin(eamm_ctx* ctx, const float* source, int n, const float* kp_driving_value, const float* kp_driving_jacobian,
                     const float* kp_source_value, const float* kp_source_jacobian, const eamm_bn_site* sites, int nsites,
                     float momentum, float eps, int sync, float* sums_buffer, const eamm_outputs* outputs, void* stream);
int eamm_train_next(eamm_ctx* ctx, int* nfloats);

/*
 * Stage timing for roofline accounting (bench.py): while enabled, every eamm_forward_frames call
 * records HIP events on the caller's stream at its stage boundaries and around every bottleneck launch
 * (up to 256 calls between reads).  eamm_profile_read waits for the recorded calls and returns
 * accumulated milliseconds per stage: 0 key points + motion front end, 1 hourglass encoder, 2 hourglass
 * decoder, 3 flow head, 4 feature warp, 5 bottleneck Winograd input transforms (0 in the direct form),
 * 6 rest of the bottleneck stage (the convolution kernels; with several chains: the stage's wall time minus the main
 * stream's transforms), 7 up blocks, 8 final 7x7 + sigmoid (+ uint8 packing) -- stages 0..8 add up to the call --
 * and 9 the bottleneck GEMM kernels' own durations on the main stream (2 x num_bottleneck_blocks launches per call;
 * with K chains each of those launches covers 1/K of the frames and runs beside the other chains' launches).
 * Chip-level accounting (all chains, not only the main stream): 10 the wall time during which ANY whole-pass chain is
 * inside its bottleneck stage (union of the chains' windows, events on every chain's stream), 11 the sum of those
 * windows, 12 executed matrix-core GFLOP of the recorded calls (what the grids really issue: padded tiles, Winograd /
 * polyphase point counts), 13 the bottleneck GEMMs' share of 12, 14..21 the same count per stage interval (key points +
 * front end, hourglass encoder, hourglass decoder, flow head, warp, bottleneck, up blocks, final layer) so that every stage's
 * fraction of the matrix peak can be printed, not only the bottleneck's.  (12..21 are GFLOP, not milliseconds.)
 */
#define EAMM_NSTAGE 22
int eamm_profile_enable(eamm_ctx* ctx, int on);
int eamm_profile_read(eamm_ctx* ctx, double* stage_ms, int nstage, int64_t* calls, int64_t* frames, int reset);

/*
 * Op-level entry points used by the parity tests (tests/test_gpu_ops.py): each runs ONE kernel of
 * the path on caller-provided device buffers so it can be compared with the oracle in isolation.
 */

/* KHxKW (3x3, 7x7 or 7x1; 1x1 on tile codes 0 / 32 / 64 / 128 with up = 0, see eamm_op_conv_ex) convolution on NHWC activations as an
 * fp32-MFMA implicit GEMM.
 * in0/in1: [B,Hin,Win,C0|C1] (in1 optional: channel concatenation), weight: OIHW host pointer
 * [Cout,C0+C1,kh,kw], bias host [Cout]; up = 1 (3x3 only) computes conv3x3(nearest_x2(input)) in its
 * collapsed four-phase 2x2 form; act: 0 none, 1 relu, 2 sigmoid; pool = 1 applies avgpool2x2 after the
 * activation; resid: NHWC tensor added before the activation; splitk 0 = automatic.  tile_n picks the kernel, with the
 * weights packed as the engine packs them for it:
 *   0                automatic register-staged tile; 32 / 64 / 128: the register-staged 128 x tile_n kernel
 *   1000 + id        LDS-DMA tile (1: 256x256, 2: 256x128, 3: 512x64, 4: 32x128, 5: 64x128); not 7x7 / 7x1
 *   2000             Winograd F(2x2,3x3): input transform + GEMM (3x3, single input, Cin % 64 == 0, no pool)
 *   2100 + variant   Winograd F(4x4,3x3) (as 2000, Hin and Win multiples of 4); variant 0 | 3 | 6: the GEMM's software pipeline
 *   2150 + groups    F(4x4,3x3) with the transform-point rows split over 2, 3 or 6 workgroups + output-transform
 *                    kernel (pool allowed without resid)
 *   3000 / 3003      spatial-patch kernel of the up-convolution (up = 1): collapsed-phase / polyphase form.  3003 is the
 *                    polyphase form as the engine runs a decoder up block: whole-tile launches form every product as six
 *                    bf16 MFMAs on exact three-way bf16 splits of the fp32 operands (fp32-exact to 2^-24 relative);
 *                    splitk > 1 splits the channel reduction over workgroups and keeps the fp32 MFMA
 *   3004             the polyphase form with fp32-MFMA products forced (splitk as 3003)
 *   4000 / 4001      column-patch kernel of a row-split 7x1 convolution (weights [Cout][C][7][1], no bias applied, act 0):
 *                    4000 the final layer (Cout 32, C0 32 or 64, no in1), 4001 the flow head (Cout 96, two inputs)
 *   4002             the generator's final layer whole (7x7, Cout 3, act 2, C0 32 or 64, no in1: out is NCHW [B,3,H,W]) as the
 *                    engine runs it: every product as six bf16 MFMAs on exact three-way bf16 splits of the fp32 operands
 *                    (fp32-exact to 2^-24 relative; an inf input gives NaN where the fp32 form saturates the sigmoid)
 *   4003             the final layer with fp32-MFMA products forced; refuses what 4002 refuses
 * out NHWC [B,H(/2),W(/2),Cout] with H = Hin << up.  iters > 0 additionally times `iters` back-to-back launches with HIP
 * events on `stream` and stores the average milliseconds in *avg_ms; a failed launch returns EAMM_ERR_HIP and stores
 * no time. */
int eamm_op_conv(int device, const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int up,
                 const float* weight_host, const float* bias_host, int Cout, int kh, int kw,
                 int act, int pool, const float* resid, int splitk, int tile_n, float* out, int iters,
                 float* avg_ms, void* stream);

/* eamm_op_conv with the operands that only the engine sets (eamm_op_conv is this call with all seven zero; tests/test_gpu_conv_modes.py):
 *   pre_scale, pre_shift   device [C0], both or neither: the Winograd input transform applies the ResBlock pre-activation
 *                          relu(x * pre_scale + pre_shift) first; the halo stays zero padding of the ACTIVATED tensor.  Tile codes
 *                          2000 and 21xx only.
 *   out2, scale2, shift2   second output relu(out * scale2 + shift2), NHWC like out (the next block's pre-activation); scale2,
 *                          shift2 device [Cout], both with out2.
 *   nchw                   1: out is written [B,Cout,H,W].
 *   split_n                > 0: channels n < split_n go to out as NHWC with a split_n-float pixel stride, channels split_n <= n <
 *                          Cout to out2 as one float4 per pixel (floats past Cout - split_n are not written); needs out2 (scale2,
 *                          shift2 unused), no resid / pool / nchw, split_n < Cout <= split_n + 4.
 *   The last five: the implicit GEMM only (tile codes 0, 32, 64, 128, 1001..1005).
 * kh = kw = 1 (a dense layer on a 1x1 map, or a pointwise convolution) is accepted on the register-staged kernel (tile codes 0, 32,
 * 64, 128) with up = 0.  pool combines with none of resid, nchw, out2, split_n.  pre_scale, pre_shift, out2, scale2 and shift2 are
 * 16-byte aligned (the kernels access them four floats at a time).  Every rule above is checked before any device work: EAMM_ERR_ARG,
 * message in eamm_last_error(NULL). */
int eamm_op_conv_ex(int device, const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int up,
                    const float* weight_host, const float* bias_host, int Cout, int kh, int kw,
                    int act, int pool, const float* resid, int splitk, int tile_n, float* out, int iters,
                    float* avg_ms, const float* pre_scale, const float* pre_shift, float* out2, const float* scale2,
                    const float* shift2, int nchw, int split_n, void* stream);

/* The host packing behind tile code 4002, no device involved: weight_host [3][C][7][7] (C = 32 | 64) -> rowsplit [21][C][7], the
 * 7x1 filter with n = dx * 3 + co the fp32 kernels' image is packed from, and planes, eamm_final_split_planes_elems(C) uint16: its
 * three bf16 planes [C/16][tap 7][plane 3][k octet 2][row n 21][8] (channel = 16 group + 8 octet + element), zero-padded to whole
 * KiB.  Plane values are the top halves of fp32 numbers whose sum is the rowsplit weight bit for bit. */
size_t eamm_final_split_planes_elems(int C);
int eamm_final_split_planes(const float* weight_host, int C, float* rowsplit, uint16_t* planes);

/* The Winograd input transform of the 3x3 / pad 1 convolution on its own, as the engine launches it: x NHWC [B,H,W,C] ->
 * V[(tile + 2)^2][B * H/tile * W/tile][C] = B^T d B of every (tile + 2)^2 patch d (stride tile, one pixel of zero padding), tile = 2
 * (F(2x2,3x3)) or 4 (F(4x4,3x3)); with scale / shift (device [C], both or neither) d is taken from relu(x * scale + shift), the
 * padding staying zero.  H, W multiples of tile, C of 4, pointers 16-byte aligned, fewer than 2^31 output elements; EAMM_ERR_ARG
 * before any launch otherwise.  Stream-ordered, no sync. */
int eamm_op_wino_transform(int device, const float* x, const float* scale, const float* shift, int B, int H, int W, int C, int tile,
                           float* V, void* stream);

/* Temporal smoothing of a clip's key points: the reference's filter1.OneEuroFilter (filter1.py:13-47)
 * applied as `process(x * scale) / scale` frame after frame (demo.py:241-250; key points: mincutoff 0.05, beta 8, dcutoff 1,
 * freq 100, scale 10; emotion displacements demo.py:231-239: 1, 0.2, 1, 100, 100).  x, out: device [T,E] float32, the filter
 * runs along T independently per element (E = K*2 values or K*4 jacobian entries; out may alias x).  `state` (device [3,E] or
 * NULL) receives the filter's memory after the last frame; with `resume` != 0 it is read first, so a clip filtered in chunks gives
 * exactly the clip filtered whole (the filter is causal: the streaming clip pipeline).  Stream-ordered, no sync. */
int eamm_op_one_euro(int device, const float* x, int T, int E, float mincutoff, float beta, float dcutoff, float freq, float scale,
                     float* out, float* state, int resume, void* stream);

/* The reference's audio front end (demo.py:314-318): python_speech_features.mfcc(signal, 16000, winstep=0.01) with the package's
 * defaults (pre-emphasis 0.97, 400-sample frames every 160 samples, rectangular window, 512-point power spectrum, 26 mel filters
 * over 0..8000 Hz, log, orthonormal DCT-II keeping 13, lifter 22, coefficient 0 replaced by the log frame energy) of a signal
 * padded with `pad` zeros on each side (1920 in the demo; the zeros are not materialised).  eamm_op_mfcc_frames gives the frame
 * count F: 1 for n_samples + 2 pad <= 400, else 1 + ceil((n_samples + 2 pad - 400) / 160); 0 for n_samples < 1 or pad < 0.
 * pcm: device float32 [n_clips][clip_stride] (the first n_samples of each row are the clip), out: device float32
 * [n_clips][F][13].  A frame's row depends on its own samples only, bit for bit.  EAMM_ERR_ARG (message in
 * eamm_last_error(NULL)) for n_samples < 1, n_clips < 1 or > 65535, pad < 0 or clip_stride < n_samples with several clips.
 * Stream-ordered, no sync. */
int64_t eamm_op_mfcc_frames(int64_t n_samples, int pad);
int eamm_op_mfcc(int device, const float* pcm, int64_t n_samples, int n_clips, int64_t clip_stride, int pad, float* out, void* stream);

/* The emotion video's preprocessing (demo.py:490 resize, demo.py:146-182 get_aligned_image, augmentation.py:403-431 with the
 * shipped config, demo.py:433-454 crop_image).  Frames are HWC uint8, coordinates (x = column, y = row); every output is
 * 256 x 256; all arithmetic after the inputs is float64 (eamm_amd/video_input.py holds the numpy oracle of every step).  Device
 * pointers unless said otherwise; stream-ordered, no sync.  EAMM_ERR_ARG (message in eamm_last_error(NULL)) before any launch
 * for a bad shape.
 *
 * eamm_op_resize_aa: in [n,H,W,C] (C = 3 | 4, alpha dropped) -> out [n,256,256,3] = trunc(255 v), v = the linear zoom
 *   (in = (o + 0.5) H / 256 - 0.5, neighbours mirrored) of the image x / 255 blurred along rows, then along columns, by the
 *   normalised Gaussian taps taps_y [2 ry + 1] / taps_x [2 rx + 1] (HOST arrays; ry, rx < 32; r = 0 with {1.0}: no blur) with
 *   'mirror' borders.  skimage.transform.resize(anti_aliasing=True) of one frame, then demo.py:162's uint8 truncation.
 * eamm_op_similarity_warp: in [n,H,W,C], maps [n][6] float64 -> output pixel (x, y) samples frame i at
 *   (maps[0] x + maps[1] y + maps[2], maps[3] x + maps[4] y + maps[5]) bilinearly (floor / ceil neighbours, a neighbour outside
 *   reads 0; skimage warp order 1, mode 'constant').  mode 0: out float32 NHWC [n,256,256,3] (the aligned video); mode 1: out
 *   float32 NCHW [n,3,256,256] = trunc(255 v) / 255 (the cropped portrait).
 * eamm_op_emotion_augment: aligned float32 NHWC [n_src,256,256,3] -> out float32 NCHW [count,3,256,256], output frame t0 + t
 *   from source frame (t0 + t) mod n_src:
 *     S2 the rectangle rows mouth_y .. + mouth_h, columns mouth_x .. + mouth_w replaced by noise: noise [n_src][mouth_h][mouth_w][3]
 *        float32, or, with noise NULL, the device hash
 *            key = mix64(noise_seed + G),  u = mix64(key + ((src * mouth_h * mouth_w + row * mouth_w + col) * 3 + ch + 1) * G) >> 40,
 *            value = u * 2^-24 (float32),  G = 0x9E3779B97F4A7C15, mix64 = the splitmix64 finaliser (uint64 arithmetic)
 *     S3 flip != 0: horizontal flip;  S4 bilinear sample at rot (HOST [6], 2 x 3) (x, y, 1), zero outside (skimage rotate);
 *     S5 hinv [n_src][9] (the inverse homography, row-major): X0, Y0, W = hinv (x, y, 1), X = rint(X0 * (32 / W)), likewise Y;
 *        neighbours (X >> 5, Y >> 5) .. + 1, each clamped to the image, weights (32 - fx)(32 - fy) / 1024 ... with fx = X & 31
 *        (cv2.warpPerspective, BORDER_REPLICATE);
 *     S6 min(255, max(0, rint(255 v))) / 255 as float32. */
int eamm_op_resize_aa(int device, const uint8_t* in, int n, int H, int W, int C, const double* taps_y, int ry, const double* taps_x,
                      int rx, uint8_t* out, void* stream);
int eamm_op_similarity_warp(int device, const uint8_t* in, int n, int H, int W, int C, const double* maps, int mode, void* out,
                            void* stream);
int eamm_op_emotion_augment(int device, const float* aligned, int64_t n_src, int64_t t0, int count, int flip, const double* rot,
                            const double* hinv, const float* noise, uint64_t noise_seed, int mouth_x, int mouth_y, int mouth_w,
                            int mouth_h, float* out, void* stream);

/* The HBM-bound kernel of the path on its own: out = grid_sample(feat, deformation, bilinear, zeros, align_corners=False)
 * * occlusion (reference modules/generator.py:50-57, 79-84).  feat: NHWC [ns,hf,wf,C] (ns = 1 broadcasts one source to
 * all frames, else ns = n), deformation [n,h,w,2], occlusion [n,h,w] or NULL, out NHWC [n,hf,wf,C]; when (h,w) != (hf,wf)
 * flow and occlusion are resized bilinearly first (generator.py:52-56, 82-83).  iters > 0 times `iters` back-to-back
 * launches with HIP events on `stream` (bench.py's isolated roofline_warp figure). */
int eamm_op_warp(int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf,
                 int wf, int C, int h, int w, float* out, int iters, float* avg_ms, void* stream);
/* eamm_op_warp (which is this call with the three NULL) with the kernel's second output out2 = relu(out * scale2 + shift2), NHWC like
 * out: the first ResBlock's pre-activation in the direct bottleneck form.  scale2, shift2: device [C]; all three or none. */
int eamm_op_warp_ex(int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf,
                    int wf, int C, int h, int w, float* out, int iters, float* avg_ms, float* out2, const float* scale2,
                    const float* shift2, void* stream);

/*
 * Backward kernels of the path's two operator kinds, op level.  The reference gets these from
 * autograd (train.py:133 `loss.backward()` through modules/generator.py and modules/util.py); the BatchNorm backward is
 * eamm_bn_backward_* above.
 */

/* Gradient of eamm_op_warp at (h,w) == (hf,wf): grad_out NHWC [n,hf,wf,C] -> grad_feat [ns,hf,wf,C] (ns = 1: summed over the
 * frames), grad_deformation [n,hf,wf,2], grad_occlusion [n,hf,wf]; any of the three may be NULL (not wanted), occlusion NULL
 * means the forward had none.  What autograd derives for F.grid_sample(bilinear, zeros, align_corners=False) * occlusion
 * (generator.py:50-57, 79-84).  The entry zeroes the gradients on `stream`, then accumulates with float atomics (grad_feat is
 * therefore equal to the fixed-order sum up to fp32 rounding of the order, as ATen's own grid_sampler backward is). */
int eamm_op_warp_backward(int device, const float* feat, const float* deformation, const float* occlusion, const float* grad_out,
                          int n, int ns, int hf, int wf, int C, float* grad_feat, float* grad_deformation, float* grad_occlusion,
                          void* stream);

/* Weight and bias gradient of a stride-1 "same" KHxKW convolution (every Conv2d of modules/util.py:858-938): x NHWC
 * [B,H,W,Cin], grad_out NHWC [B,H,W,Cout] -> grad_weight OIHW [Cout,Cin,kh,kw] (device), grad_bias [Cout] (device, or NULL).
 * fp32-MFMA GEMMs with K = the B*H*W pixels split over workgroups, partial sums in `workspace`
 * (eamm_op_conv_wgrad_workspace_floats floats for this shape) and summed in a fixed order: deterministic.  Forms: Winograd
 * F(3x3,4x4) for 3x3 filters on maps with sides multiples of 4 and at least 512 tiles (36 GEMMs over the tiles on the forward's
 * transformed input: a quarter of the multiplies), one GEMM per filter ROW for maps with W % 32 == 0, else one per tap.
 * Cin, Cout multiples of 4, Cout <= 1024; kh, kw odd and at most 7.  The DATA gradient of such a convolution is eamm_op_conv on grad_out with the filter transposed and
 * flipped (weight.permute(1,0,2,3).flip(2,3)), which eamm_amd/autograd_ops.py does. */
/* Stride-1 "same" 1x1 / 3x3 / 7x7 convolution with DEVICE parameters (the training path: they change every optimiser step):
 * x NHWC [B,H,W,Cin], weight OIHW [Cout,Cin,kh,kw] and bias [Cout] (or NULL) in device memory, out NHWC [B,H,W,Cout].  The filter
 * is packed on the device into `workspace` (eamm_op_conv_dev_workspace_floats floats, 16-byte aligned) and the evaluation
 * path's kernels run on it: F(4x4,3x3) Winograd where the bottleneck's kernel applies (3x3, Cin % 64 == 0, H and W multiples of
 * 4, >= 2048 tiles), else the register-staged implicit GEMM.  transposed = 1 computes the DATA GRADIENT of such a convolution:
 * x is then grad_out [B,H,W,Cin = the forward's Cout], weight the FORWARD filter [Cin,Cout,kh,kw], read transposed over
 * (out, in) and flipped over (y, x) while packing.  Asynchronous on `stream`; Cin a multiple of 32, Cout of 4. */
size_t eamm_op_conv_dev_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw);
int eamm_op_conv_dev(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int kh,
                     int kw, int transposed, float* out, float* workspace, size_t workspace_floats, void* stream);

/* The generator's two 7x7 layers with THREE channels on one side (`first` 3 -> N, `final` N -> 3: reference
 * modules/generator.py:26, 48), training path, without padding the thin side to 32 channels.  Thin tensors are NHWC with FOUR
 * floats per pixel, [B,H,W,4], the fourth zero; N = 32 | 64; device pointers; `workspace` of eamm_op_conv7_thin_workspace_floats.
 *   eamm_op_conv7_thin        transposed = 0: out [B,H,W,N] = conv7x7_same(thin, weight [N,3,7,7]) + bias   (forward of `first`)
 *                             transposed = 1: out [B,H,W,N] = data gradient of y3 = conv7x7_same(x [.,N], weight [3,N,7,7]) from
 *                                             thin = d y3                                                  (backward of `final`)
 *   eamm_op_conv7_thin_wgrad  thin_is_input = 1: grad_weight [N,3,7,7] from thin = the layer's input, wide = d out [B,H,W,N]
 *                             thin_is_input = 0: grad_weight [3,N,7,7] from thin = d y3, wide = the layer's input [B,H,W,N]
 * (the forward of `final` is the evaluation path's column-patch kernel: eamm_op_conv tile 4002; bias gradients: eamm_op_conv_wgrad's
 * or a plain sum). */
size_t eamm_op_conv7_thin_workspace_floats(int B, int H, int W, int N);
int eamm_op_conv7_thin(int device, const float* thin, const float* weight, const float* bias, int B, int H, int W, int N, int transposed,
                       float* out, float* workspace, size_t workspace_floats, void* stream);
int eamm_op_conv7_thin_wgrad(int device, const float* thin, const float* wide, int B, int H, int W, int N, int thin_is_input,
                             float* grad_weight, float* workspace, size_t workspace_floats, void* stream);

/* The generator's last layer whole with DEVICE parameters (training path): out NCHW [B,3,H,W] = sigmoid(conv7x7_same(x [B,H,W,C],
 * weight [3,C,7,7]) + bias [3]) -- reference modules/generator.py:92-93 -- on the evaluation path's fused column-patch kernel;
 * the filter is packed on the device into `workspace` (7 * C * 32 floats, 16-byte aligned).  C = 32 | 64. */
int eamm_op_final_conv_sigmoid(int device, const float* x, const float* weight, const float* bias, int B, int H, int W, int C,
                               float* out_nchw, float* workspace, size_t workspace_floats, void* stream);

size_t eamm_op_conv_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw);
int eamm_op_conv_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                       float* grad_weight, float* grad_bias, float* workspace, size_t workspace_floats, void* stream);
/* Where eamm_op_conv_dev ran the F(4x4,3x3) form AND the weight gradient takes its F(3x3,4x4) form, both start from the same
 * transformed input V = B^T x B: a caller that keeps the forward call's workspace alive until the backward (autograd's saved
 * tensors) passes workspace + eamm_op_conv_saved_transform_offset(...) as `x_transformed` and the transform is not run again
 * (2.25 x the activation kept instead of 1 x; the same sums in the same order: bit-identical to eamm_op_conv_wgrad).
 * The offset is (size_t)-1 for a shape without a shared transform.  Workspace: eamm_op_conv_wgrad_workspace_floats. */
size_t eamm_op_conv_saved_transform_offset(int B, int H, int W, int Cin, int Cout, int kh, int kw);
int eamm_op_conv_wgrad_saved(int device, const float* x_transformed, const float* grad_out, int B, int H, int W, int Cin, int Cout,
                             float* grad_weight, float* grad_bias, float* workspace, size_t workspace_floats, void* stream);

/*
 * The dense-motion front end and flow head as DIFFERENTIABLE operators (round 4): forward = the evaluation
 * path's kernels (motion.hip), backward = what autograd derives from the reference's torch ops (motion_backward.hip).  Device
 * pointers, per-pair sources (n sources for n driving frames, the training batch of train.py:133); asynchronous on `stream`.
 *   eamm_op_antialias_down            AntiAliasInterpolation2d (modules/util.py:1044-1052): source NCHW [B,3,H,W], the module's
 *                                     [3,1,13,13] buffer -> small NHWC [B,H/s,W/s,4] (RGB + a zero); inv_scale 4 (scale_factor 0.25)
 *                                     or 1 (a copy, util.py:1047-1048); the forward also takes 2 (the same buffer: its sigma is fixed)
 *   eamm_op_antialias_down_backward   grad_small [B,h,w,4] -> grad_source [B,3,H,W]; inv_scale 4 | 1
 *   eamm_op_kp_records                records [n,K,8] = kp_driving.xy, kp_source.xy, J = jac_source inverse(jac_driving)
 *                                     (dense_motion.py:47-67; jacobians NULL: identity); *singular_flag (device int) is set when
 *                                     a driving jacobian is singular (torch.inverse raises)
 *   eamm_op_kp_records_backward       grad_records -> grad of the four key-point tensors (any may be NULL)
 *   eamm_op_motion_front              heat-maps (util.py:815-836, dense_motion.py:32-45), sparse motions and the K+1 warps of
 *                                     `small` (:69-79) -> hourglass_in NHWC [n,h,w,Cpad] (channel 4k heat-map k, 4k+1..3 RGB warped
 *                                     by motion k, zero padded; dense_motion.py:93-94) and sparse_deformed [n,K+1,3,h,w] (or NULL)
 *   eamm_op_motion_front_backward     grad of both outputs (either may be NULL) -> grad_small [n,h,w,4] (or NULL; float atomics like
 *                                     ATen's grid_sampler backward) and grad_records [n,K,8] (fixed-order sums: deterministic)
 *   eamm_op_motion_head               mask = softmax over the K+1 mask logits [n,h,w,ld], deformation = sum_k mask_k T_k,
 *                                     occlusion = sigmoid(logit [n,h,w,ldo] channel 0) (dense_motion.py:98-111; occlusion NULL: none)
 *   eamm_op_motion_head_backward      grad_mask [n,K+1,h,w], grad_deformation [n,h,w,2], grad_occlusion [n,h,w] (any may be NULL)
 *                                     -> grad of the logits (same layouts, unused channels zeroed) and grad_records.
 *                                     Stacked logits (ONE convolution producing mask and occlusion: occlusion_logits =
 *                                     mask_logits + K + 1, ldo = ld; the same for the two gradient pointers) are recognised: the
 *                                     occlusion logit's gradient then lands in channel K + 1 of the one gradient tensor
 * `workspace`: eamm_op_motion_workspace_floats(n, K, h, w) floats.
 */
int eamm_op_antialias_down(int device, const float* source, const float* aa_weight, int B, int H, int W, int inv_scale, float* small,
                           void* stream);
int eamm_op_antialias_down_backward(int device, const float* grad_small, const float* aa_weight, int B, int H, int W, int inv_scale,
                                    float* grad_source, void* stream);
int eamm_op_kp_records(int device, const float* kd_val, const float* kd_jac, const float* ks_val, const float* ks_jac, int n, int K,
                       float* records, int* singular_flag, void* stream);
int eamm_op_kp_records_backward(int device, const float* kd_jac, const float* ks_jac, const float* grad_records, int n, int K,
                                float* grad_kd_val, float* grad_ks_val, float* grad_kd_jac, float* grad_ks_jac, void* stream);
size_t eamm_op_motion_workspace_floats(int n, int K, int h, int w);
int eamm_op_motion_front(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance, int Cpad,
                         float* hourglass_in, float* sparse_deformed, void* stream);
int eamm_op_motion_front_backward(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance,
                                  int Cpad, const float* grad_hourglass_in, const float* grad_sparse_deformed, float* grad_small,
                                  float* grad_records, float* workspace, size_t workspace_floats, void* stream);
int eamm_op_motion_head(int device, const float* mask_logits, int ld, const float* occlusion_logits, int ldo, const float* records, int n,
                        int K, int h, int w, float* mask, float* deformation, float* occlusion, void* stream);
int eamm_op_motion_head_backward(int device, const float* mask, const float* occlusion, const float* records, int n, int K, int h, int w,
                                 const float* grad_mask, const float* grad_deformation, const float* grad_occlusion,
                                 float* grad_mask_logits, int ld, float* grad_occlusion_logits, int ldo, float* grad_records,
                                 float* workspace, size_t workspace_floats, void* stream);

/*
 * The key-point heads' reduction as a DIFFERENTIABLE operator (reference modules/keypoint_detector.py:77-105 / :180-205): the
 * forward is the detectors' own kernels, the backward beside them (kp_head.hip).  Device pointers; asynchronous on `stream`.
 *   eamm_op_kp_head            logits NHWC [B,h,w,Cs] = the "same"-padded 7x7 convolution's output with the `kp` and `jacobian` filters
 *                              stacked: channel k is key point k's logit, channel K + 4 m + c entry c of jacobian map m (njm = 0, 1 or
 *                              K maps).  The reference convolves with padding `pad`: only the window [off, off + oh) x [off, off + ow),
 *                              off = 3 - pad, oh = h - 2 off, ow = w - 2 off, exists.  heatmap = softmax(logit / temperature) over the
 *                              window [B,K,oh,ow] (or NULL), value = sum heatmap * grid [B,K,2], jacobian = sum heatmap * map
 *                              [B,K,2,2] (or NULL), stats [B,K,2] (or NULL) = the softmax's (maximum, denominator), kept for the backward.
 *                              Always the pixel-sliced kernels with B >= 8, one workgroup per (image, key point) below, as the
 *                              detectors' inference calls: the same bits.
 *   eamm_op_kp_head_backward   g_value [B,K,2], g_jacobian [B,K,2,2], g_heatmap [B,K,oh,ow] (any may be NULL) -> grad_logits
 *                              [B,h,w,Cs], FULLY written: zeros outside the window and in the channels >= K + 4 njm.  With p the
 *                              heat-map and a_i = g_value . grid_i + sum_c g_jacobian[c] J_c,i + g_heatmap_i:
 *                                  dL/dl_i = p_i (a_i - sum_j p_j a_j) / temperature,   dL/dJ_c,i = g_jacobian[c] p_i
 *                              (njm = 1: summed over the key points in their order); sum_j p_j a_j = g_value . value +
 *                              g_jacobian . jacobian + sum_j p_j g_heatmap_j, the last term summed over pixel slices in a fixed
 *                              order (deterministic, no float atomics).  Cs a multiple of 4, 16-byte aligned tensors.
 * `workspace`: eamm_op_kp_head_workspace_floats(B, K) floats, for either call.
 */
size_t eamm_op_kp_head_workspace_floats(int B, int K);
int eamm_op_kp_head(int device, const float* logits, int B, int K, int njm, int h, int w, int Cs, int pad, float temperature, float* value,
                    float* jacobian, float* heatmap, float* stats, float* workspace, size_t workspace_floats, void* stream);
int eamm_op_kp_head_backward(int device, const float* logits, const float* stats, const float* value, const float* jacobian,
                             const float* g_value, const float* g_jacobian, const float* g_heatmap, int B, int K, int njm, int h, int w, int Cs,
                             int pad, float temperature, float* grad_logits, float* workspace, size_t workspace_floats, void* stream);

/*
 * The stride-2 convolution of Emotion_k's ResNet-18 trunk as a DIFFERENTIABLE operator (reference modules/util.py:1069-1099: the first
 * 3x3 convolution of a down-sampling BasicBlock and its 1x1 `downsample` shortcut).  Additive entries (ABI 6 unchanged).  Common
 * contract: NHWC fp32 activations, OIHW filter [Cout,Cin,k,k] ON THE DEVICE with k 1 | 3, padding k / 2, no bias; Hin and Win
 * even; Cin and Cout multiples of 32; anything else is refused before any launch and the *_workspace_floats query returns 0.
 * `workspace`: the query's floats, 16-byte aligned (the packed filter and the split slabs live there).  Asynchronous on `stream`.
 *   eamm_op_conv_s2        x [B,Hin,Win,Cin] -> out [B,Hin/2,Win/2,Cout]: the emotion engine's fp32-MFMA kernel (conv_s2.hip) on a
 *                          filter packed on the device.
 *   eamm_op_conv_s2_dgrad  grad_out [B,Hin/2,Win/2,Cout], weight -> grad_x [B,Hin,Win,Cin], a gather: one implicit GEMM on
 *                          v_mfma_f32_32x32x2_f32 per input-pixel parity class (1, 2, 2 or 4 of the nine taps reach a pixel; for k = 1
 *                          only the even / even pixels).  No atomics; EVERY element is written (exact zeros where no tap reaches);
 *                          bit-identical from run to run.
 *   eamm_op_conv_s2_wgrad  x, grad_out -> grad_weight [Cout,Cin,k,k]: one GEMM per tap over the output pixels, split over the pixel
 *                          range, the slabs summed in a fixed order (deterministic).
 */
size_t eamm_op_conv_s2_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k);
int eamm_op_conv_s2(int device, const float* x, int B, int Hin, int Win, int Cin, const float* weight, int Cout, int k, float* out,
                    float* workspace, size_t workspace_floats, void* stream);
size_t eamm_op_conv_s2_dgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k);
int eamm_op_conv_s2_dgrad(int device, const float* grad_out, int B, int Hin, int Win, int Cin, const float* weight, int Cout, int k,
                          float* grad_x, float* workspace, size_t workspace_floats, void* stream);
size_t eamm_op_conv_s2_wgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k);
int eamm_op_conv_s2_wgrad(int device, const float* x, const float* grad_out, int B, int Hin, int Win, int Cin, int Cout, int k,
                          float* grad_weight, float* workspace, size_t workspace_floats, void* stream);

/*
 * Emotion_k's small steps as DIFFERENTIABLE operators (reference modules/util.py:1245, :1287-1295).  Device pointers; asynchronous.
 *   eamm_op_emo_maxpool           MaxPool2d(3, 2, 1) on NHWC x [B,H,W,C] (H, W even) -> out [B,H/2,W/2,C].
 *   eamm_op_emo_maxpool_backward  grad_x [B,H,W,C], fully written: the winner of each window is recomputed from x; the FIRST maximum
 *                                 in (ky, kx) raster order takes the gradient (ATen's rule); each input pixel sums the up-to-four
 *                                 windows that chose it (no atomics).
 *   eamm_op_emo_final             the `final` stack Conv1d(1,2,4,2,1) - MaxPool1d(2,2) - ReLU - Conv1d(2,4,4,2,1) - ReLU - Conv1d(4,4,3)
 *                                 on a [B,64] -> value [B,4,2], jacobian [B,4,2,2] (either may be NULL); w98 = the six parameter
 *                                 tensors flattened in state_dict order (8 + 2 + 32 + 4 + 48 + 4 floats).
 *   eamm_op_emo_final_backward    g_value, g_jacobian (either may be NULL) -> grad_a [B,64] and grad_w98 [98], summed over the frames
 *                                 in their order; workspace: eamm_op_emo_final_workspace_floats(B) floats.
 */
int eamm_op_emo_maxpool(int device, const float* x, int B, int H, int W, int C, float* out, void* stream);
int eamm_op_emo_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, float* grad_x, void* stream);
int eamm_op_emo_final(int device, const float* a, const float* w98, int B, float* value, float* jacobian, void* stream);
size_t eamm_op_emo_final_workspace_floats(int B);
int eamm_op_emo_final_backward(int device, const float* a, const float* w98, const float* g_value, const float* g_jacobian, int B,
                               float* grad_a, float* grad_w98, float* workspace, size_t workspace_floats, void* stream);

/*
 * AT_net2's LSTM layer, max-pools and ConvTranspose2d(k4, s2, p1) as DIFFERENTIABLE operators (reference modules/util.py:539-576,
 * :596-598; what train.py's first stage back-propagates through).  Additive entries (ABI 6 unchanged).  Device pointers, fp32;
 * asynchronous on `stream`; a bad shape is refused before any launch and the *_workspace_floats query returns 0 for it.
 * `workspace`: the query's floats, 16-byte aligned.
 *   eamm_op_lstm_forward    one nn.LSTM layer (hidden 256, gates i f g o) from a zero state: xproj [N,T,1024] = x W_ih^T + b_ih + b_hh,
 *                           w_hh [1024,256] -> y [N,T,256]; 1 <= N <= 8, T >= 1.  The inference engine's persistent recurrence
 *                           kernel, on a W_hh image packed on the device; the call zeroes its own hand-off words on the stream.
 *   eamm_op_lstm_scan       gate pre-activations [N,T,1024] -> the activated gates IN PLACE and the cell states c [N,T,256].
 *   eamm_op_lstm_backward   acts, c (eamm_op_lstm_scan), w_hh, grad_y [N,T,256] -> grad_xproj [N,T,1024] (= the gate gradients): one
 *                           persistent launch of 16 workgroups stepping t = T-1 .. 0, each owning 16 hidden units with its
 *                           1024 x 16 slice of W_hh in LDS, exchanging the gate gradients of a step through tagged 8-byte words.
 *   eamm_op_lstm_check      waits for `stream`; EAMM_ERR_HIP if a recurrence of either direction timed out on this device (a
 *                           workgroup waited more than 10 s for another): the outputs hold NaN from the step it stopped at, and
 *                           the LSTM operators of the device refuse further calls.
 *   eamm_op_audio_maxpool / _backward   MaxPool2d(3, (sy, sx)) without padding on NHWC x [B,H,W,C] (C a multiple of 4, strides 1 | 2)
 *                           -> [B,(H-3)/sy+1,(W-3)/sx+1,C]; backward: grad_x fully written, a gather per input pixel over the windows
 *                           that contain it, each window's winner recomputed (first maximum in row-major order); no atomics.
 *   eamm_op_deconv4s2       ConvTranspose2d(Cin, Cout, 4, 2, 1): x [B,H,W,Cin], weight [Cin,Cout,4,4] (the reference's layout), bias
 *                           [Cout] or NULL -> out [B,2H,2W,Cout]; Cin and Cout multiples of 32.  The four-phase 2x2 form: one
 *                           implicit GEMM on v_mfma_f32_32x32x2_f32 per output-pixel parity class.
 *   eamm_op_deconv4s2_dgrad grad_out [B,2H,2W,Cout], weight -> grad_x [B,H,W,Cin]: the 4x4 stride-2 pad-1 convolution of grad_out as a
 *                           gather per input pixel on the matrix cores; no atomics, every element written.
 *   eamm_op_deconv4s2_wgrad x, grad_out -> grad_weight [Cin,Cout,4,4] (one GEMM per tap, split over the pixels, the slabs summed in
 *                           a fixed order) and, unless NULL, grad_bias [Cout].
 */
size_t eamm_op_lstm_workspace_floats(int N, int T);
int eamm_op_lstm_forward(int device, const float* xproj, const float* w_hh, int N, int T, float* y, float* workspace, size_t workspace_floats,
                         void* stream);
int eamm_op_lstm_scan(int device, float* gates, int N, int T, float* c, void* stream);
size_t eamm_op_lstm_backward_workspace_floats(int N, int T);
int eamm_op_lstm_backward(int device, const float* acts, const float* c, const float* w_hh, const float* grad_y, int N, int T,
                          float* grad_xproj, float* workspace, size_t workspace_floats, void* stream);
int eamm_op_lstm_check(int device, void* stream);
int eamm_op_audio_maxpool(int device, const float* x, int B, int H, int W, int C, int sy, int sx, float* out, void* stream);
int eamm_op_audio_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, int sy, int sx,
                                   float* grad_x, void* stream);
size_t eamm_op_deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout);
int eamm_op_deconv4s2(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, float* out,
                      float* workspace, size_t workspace_floats, void* stream);
size_t eamm_op_deconv4s2_dgrad_workspace_floats(int B, int H, int W, int Cin, int Cout);
int eamm_op_deconv4s2_dgrad(int device, const float* grad_out, int B, int H, int W, int Cin, const float* weight, int Cout, float* grad_x,
                            float* workspace, size_t workspace_floats, void* stream);
size_t eamm_op_deconv4s2_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout);
int eamm_op_deconv4s2_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, float* grad_weight,
                            float* grad_bias, float* workspace, size_t workspace_floats, void* stream);

/*
 * The frozen inference path's small kernels at OPERATOR level: one launch each of what the engines run per frame or once per clip,
 * on the caller's device buffers (the tests compare each with a float64 reference at shapes the whole-model fixtures do not
 * reach).  Additive entries (ABI 6 unchanged).  fp32, device pointers unless named *_host; asynchronous on `stream`; a bad argument
 * is refused with EAMM_ERR_ARG before any launch.
 *   eamm_op_first7                the generator's first block, relu(conv7x7_same(source NCHW [ns,3,H,W], w_host [Cout,3,7,7]) + b_host
 *                                 [Cout]) -> out NHWC [ns,H,W,Cout] on the dedicated 3-channel kernel; the HOST filter (BatchNorm
 *                                 folded) is packed as the engine packs it; Cout 32 | 64 | 96 | 128.  Waits for `stream` before it
 *                                 returns (it frees its packed filter).
 *   eamm_op_motion_head_infer     the flow head's inference kernel on logits NHWC [n,h,w,32] (channels 0..K the mask logits, K + 1 the
 *                                 occlusion logit, the rest unread), records [n,K,8] (eamm_op_kp_records): deformation [n,h,w,2],
 *                                 occlusion [n,h,w] (has_occ), and, unless NULL, mask_out [n,K+1,h,w] and occ_out [n,1,h,w].  K <= 30.
 *   eamm_op_motion_head_rowsplit  the same from the 7x1 convolution's partial products part [n,h,w,PS], channel dx * NC + co (channels
 *                                 >= 7 NC unread): logit co = bias[co] + sum_dx part[y, x + dx - 3, dx * NC + co], zero outside the row.
 *                                 K + 1 + has_occ <= NC <= 32, PS >= 7 NC.
 *   eamm_op_final_shift_sum       out NCHW [n,3,H,W] = sigmoid(bias[co] + sum_dx part[y, x + dx - 3, dx * 3 + co]) from part [n,H,W,32]
 *                                 (channels 21..31 unread).
 *   eamm_op_to_u8                 prediction NCHW [n,3,H,W] -> out uint8 [n,H,W,3]: rint(p * 255) clamped to 0..255.
 *   eamm_op_warp_image            the `deformed` output: deformation [n,h,w,2] resized bilinearly to (H,W) unless equal, then
 *                                 grid_sample(bilinear, zeros, align_corners=False) of the first `channels` of source's src_planes
 *                                 planes, source [ns,src_planes,H,W] with ns 1 | n -> out [n,channels,H,W].
 *   eamm_op_source_prepare        once per clip: source NCHW [ns,3,H,W] -> source_nhwc [ns,H,W,Cpad] (RGB + zeros) and `small`
 *                                 [ns,H/s,W/s,4] = eamm_op_antialias_down's result; inv_scale s 1 | 2 | 4, aa_weight [3,1,13,13].
 *   eamm_op_broadcast_features    a generator without a motion network: out [n,hf,wf,C] = feat [ns,hf,wf,C] frame i (ns = n) or frame 0
 *                                 (ns = 1); out2 (or NULL) = relu(out * scale[c] + shift[c]), one fused multiply-add.  C a multiple of 4.
 *   eamm_op_nchw_to_nhwc_pad      src [B,planes,H,W] -> dst [B,H,W,Cpad]: the first C planes, zeros in channels C..Cpad-1.
 *   eamm_op_emo_avgpool           NHWC x [B,P,C] -> out [B,C], the mean over the P pixels.
 *   eamm_op_emo_embed             value [B,10,2], jacobian [B,10,2,2] -> out [B,1260]: per key point the six numbers d, then sin / cos of
 *                                 d * 2^f, f = 0..9, interleaved over the six ([d6, sin6, cos6, sin6 (2d), ...]).
 *   eamm_op_emo_linear            out [B,O] = act(bias + [x0 [B,K0] | x1 [B,K1]] wt), wt TRANSPOSED [K0+K1][O]; x1 NULL with K1 = 0;
 *                                 relu 0 | 1; K0 + K1 <= 2048.
 *   eamm_op_audio_conv1           AT_net2's first block: relu(conv3x3_same(x [F,H,W], w) + b) -> out NHWC [F,H,W,64]; w is the folded
 *                                 filter TRANSPOSED [9][64] (tap dy * 3 + dx major), b [64].
 *   eamm_op_audio_scale           x[i] *= scale in place, n floats.
 */
int eamm_op_first7(int device, const float* source, int ns, int H, int W, const float* w_host, const float* b_host, int Cout, float* out,
                   void* stream);
int eamm_op_motion_head_infer(int device, const float* logits, const float* records, int n, int K, int h, int w, int has_occ,
                              float* deformation, float* occlusion, float* mask_out, float* occ_out, void* stream);
int eamm_op_motion_head_rowsplit(int device, const float* part, int PS, int NC, const float* bias, const float* records, int n, int K, int h,
                                 int w, int has_occ, float* deformation, float* occlusion, float* mask_out, float* occ_out, void* stream);
int eamm_op_final_shift_sum(int device, const float* part, const float* bias, int n, int H, int W, float* out, void* stream);
int eamm_op_to_u8(int device, const float* prediction, int n, int H, int W, uint8_t* out, void* stream);
int eamm_op_warp_image(int device, const float* source, const float* deformation, int n, int ns, int H, int W, int h, int w, int src_planes,
                       int channels, float* out, void* stream);
int eamm_op_source_prepare(int device, const float* source, const float* aa_weight, int ns, int H, int W, int inv_scale, int Cpad,
                           float* source_nhwc, float* small, void* stream);
int eamm_op_broadcast_features(int device, const float* feat, int n, int ns, int hf, int wf, int C, float* out, float* out2, const float* scale,
                               const float* shift, void* stream);
int eamm_op_nchw_to_nhwc_pad(int device, const float* src, int B, int C, int planes, int H, int W, int Cpad, float* dst, void* stream);
int eamm_op_emo_avgpool(int device, const float* x, int B, int P, int C, float* out, void* stream);
int eamm_op_emo_embed(int device, const float* value, const float* jacobian, int B, float* out, void* stream);
int eamm_op_emo_linear(int device, const float* x0, int K0, const float* x1, int K1, const float* wt, const float* bias, int O, int B, int relu,
                       float* out, void* stream);
int eamm_op_audio_conv1(int device, const float* x, const float* w, const float* b, int F, int H, int W, float* out, void* stream);
int eamm_op_audio_scale(int device, float* x, size_t n, float scale, void* stream);

/*
 * The pyramid perceptual loss around its convolutions (reference modules/model.py:10-68, :236-248) as DIFFERENTIABLE operators
 * (perceptual.hip); VGG19's convolutions themselves are eamm_op_conv_dev.  Device pointers; asynchronous on `stream`; no float
 * atomics anywhere: every result is the same bits from run to run.
 *   eamm_op_vgg_input            one pyramid level of image NCHW [B,3,H,W]: zero-pad 6, the depth-wise [3,1,13,13] sigma-1.5 buffer,
 *                                every inv_scale-th row and column (util.py:1044-1052; inv_scale any integer >= 1 dividing H and W,
 *                                1: the image itself) -> out_nhwc [B,H/s,W/s,32]: (level - mean[c]) / std[c] in channels 0..2, exact
 *                                zeros in 3..31 (conv1_1's input), and / or level_nchw [B,3,H/s,W/s], the un-normalised level
 *                                (ImagePyramide's output).  Either output may be NULL, not both.
 *   eamm_op_vgg_input_backward   grad_nhwc [B,h,w,grad_channels] (channels 0..2 are read; grad_channels a multiple of 4: 32, or 4
 *                                from conv1_1's data gradient with the filter cut to four input channels) and / or grad_level
 *                                [B,3,h,w] -> grad_image [B,3,H,W], fully written: the transposed Gaussian as a gather.
 *   eamm_op_relu_pool            x [B,H,W,C] (C a multiple of 32) = relu(x) IN PLACE; pooled (or NULL) [B,H/2,W/2,C] =
 *                                MaxPool2d(2, 2) of it, sizes floored: an odd last row or column feeds no window.
 *   eamm_op_relu_pool_backward   dx = (y > 0) * (dy + dp routed to its window's FIRST maximum in row-major order); dy [B,H,W,C] (the
 *                                gradient arriving at y itself) and dp [B,H/2,W/2,C] may each be NULL, not both.
 *   eamm_op_l1_pair              value[0] = weight * mean|a - b| over n elements as a fixed-order two-stage sum (the order depends on
 *                                n alone), grad[n] = (weight / n) * sign(a - b) with sign(0) = 0; workspace:
 *                                eamm_op_l1_pair_workspace_floats(n) floats, 16-byte aligned.
 *   eamm_op_l1_pair_backward     out[n] = grad[n] * grad_value[0] (grad_value on the device).
 */
int eamm_op_vgg_input(int device, const float* image, const float* aa_weight, const float* mean, const float* std_, int B, int H, int W,
                      int inv_scale, float* out_nhwc, float* level_nchw, void* stream);
int eamm_op_vgg_input_backward(int device, const float* grad_nhwc, int grad_channels, const float* grad_level, const float* aa_weight,
                               const float* std_, int B, int H, int W, int inv_scale, float* grad_image, void* stream);
int eamm_op_relu_pool(int device, float* x, int B, int H, int W, int C, float* pooled, void* stream);
int eamm_op_relu_pool_backward(int device, const float* y, const float* dy, const float* dp, int B, int H, int W, int C, float* dx,
                               void* stream);
size_t eamm_op_l1_pair_workspace_floats(long long n);
int eamm_op_l1_pair(int device, const float* a, const float* b, long long n, float weight, float* value, float* grad, float* workspace,
                    size_t workspace_floats, void* stream);
int eamm_op_l1_pair_backward(int device, const float* grad, long long n, const float* grad_value, float* out, void* stream);

/*
 * The discriminator (reference modules/discriminator.py) as DIFFERENTIABLE operators, a family of its own: eamm_disc_* (disc_conv4.hip,
 * disc_norm.hip).  Device pointers, NHWC fp32 maps, 16-byte aligned; asynchronous on `stream`; the operator convention (device index
 * first, workspace pair before the stream, errors through eamm_last_error(NULL)).  No float atomics anywhere: every sum has a fixed
 * order, every result is the same bits from run to run.  The 512 -> 1 prediction layer is eamm_op_conv_dev / eamm_op_conv_wgrad (1x1).
 *   eamm_disc_conv4              valid (unpadded) stride-1 4x4 convolution: x [B,H,W,Cin], weight OIHW [Cout,Cin,4,4] and bias [Cout]
 *                                (or NULL) -> out [B,H+2pad-3,W+2pad-3,Cout] on the fp32 matrix cores (v_mfma_f32_32x32x2_f32); the
 *                                filter is packed into `workspace` on every call.  pad = 0, transposed = 0: the forward.  pad = 3,
 *                                transposed = 1: the DATA GRADIENT -- x is grad_out [B,H,W,Cin = the forward's Cout], weight the FORWARD
 *                                filter [Cin,Cout,4,4], read transposed over (out, in) and flipped over (y, x) while packing.  Cin and
 *                                Cout multiples of 32, H and W at least 4 (forward; the data gradient takes any grad_out).  thin = 4 | 8 | 16: the side with few channels (the image,
 *                                or the image with the key-point heat maps) has `thin` floats per pixel.  Forward: x [B,H,W,thin]
 *                                with exact zeros above the real channels, weight [Cout,Cin,4,4] with 1 <= Cin <= thin (K = 16 thin
 *                                instead of 16 x 32: the kx taps of a filter row are contiguous in such a map).  Data gradient:
 *                                weight [Cin,Cout,4,4] with 1 <= Cout <= thin, out [B,H+3,W+3,thin] with zeros above Cout (runs the
 *                                ordinary form on a 32-column tile).
 *   eamm_disc_conv4_wgrad        x [B,H,W,Cin] (Cin 4 | 8 | 16 for a thin input, else a multiple of 32), grad_out [B,H-3,W-3,Cout]
 *                                -> grad_weight [Cout,Cin,4,4] (or NULL: the bias gradient alone), grad_bias [Cout] (or NULL): one GEMM per tap with K = the pixels split
 *                                over workgroups, the slabs summed in slice order.  Cout a multiple of 32, at most 1024.
 *   eamm_disc_norm_act_pool      out = AvgPool2d(2)?(LeakyReLU_0.2(InstanceNorm2d(x) * gamma + beta)): x [B,H,W,C]; norm = 1: affine
 *                                InstanceNorm, eps 1e-5, biased variance, no running statistics, with stats [B,C,2] DOUBLES = (mean,
 *                                1 / sqrt(var + eps)) written for the backward (sums in double, fixed order); norm = 0: no
 *                                normalisation (gamma, beta, stats, workspace may be NULL).  pool = 1: out [B,H/2,W/2,C], sizes
 *                                floored (an odd last row or column feeds no window); pool = 0: out [B,H,W,C].  C a multiple of 4, at
 *                                most 1024; H * W >= 2 with norm (one value per channel has no variance: refused, as torch does).
 *   eamm_disc_norm_act_pool_backward  from the saved x and stats: grad_out [B,H/2,W/2,C] (pool) or [B,H,W,C] -> grad_x [B,H,W,C],
 *                                grad_gamma [C], grad_beta [C] (each may be NULL, not all; norm = 0: grad_x alone).
 * Workspaces: the *_workspace_floats query of the entry for the same shape (0: the shape is refused, or -- norm = 0 -- none is needed).
 */
size_t eamm_disc_conv4_workspace_floats(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin);
int eamm_disc_conv4(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int pad,
                    int transposed, int thin, float* out, float* workspace, size_t workspace_floats, void* stream);
size_t eamm_disc_conv4_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout);
int eamm_disc_conv4_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, float* grad_weight,
                          float* grad_bias, float* workspace, size_t workspace_floats, void* stream);
size_t eamm_disc_norm_act_pool_workspace_floats(int B, int H, int W, int C, int norm);
int eamm_disc_norm_act_pool(int device, const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, int norm, int pool,
                            double* stats, float* out, float* workspace, size_t workspace_floats, void* stream);
size_t eamm_disc_norm_act_pool_backward_workspace_floats(int B, int H, int W, int C, int norm);
int eamm_disc_norm_act_pool_backward(int device, const float* x, const double* stats, const float* gamma, const float* beta,
                                     const float* grad_out, int B, int H, int W, int C, int norm, int pool, float* grad_x, float* grad_gamma,
                                     float* grad_beta, float* workspace, size_t workspace_floats, void* stream);

/*
 * The equivariance constraint's random transform (reference modules/model.py:71-152, class Transform), a family of its own: eamm_equi_*
 * (equivariance.hip).  Device pointers, fp32, 4-byte aligned; asynchronous on `stream`; the operator convention (device index first,
 * stream last, errors through eamm_last_error(NULL)).  No atomics: every result is the same bits from run to run.
 *   theta [B,2,3] the affine part, control_params [B,points^2] the thin-plate weights of the points x points coordinate grid (row-major,
 *   x = 2 j / (points - 1) - 1); points = 0: affine only (control_params may be NULL), else 2..16.  For a point c = (x, y) of image b:
 *       warp(c) = theta[b,:,:2] c + theta[b,:,2] + (r, r),  r = sum_p w[b,p] U(|x - cx_p| + |y - cy_p|),  U(d) = d^2 logf(d + 1e-6)
 *   (the L1 distance, and one r for both components, are the reference's), summed over p ascending.
 *   eamm_equi_tps_warp_frame     frame NCHW [B,C,H,W] -> out [B,C,H,W] = F.grid_sample(frame, warp(make_coordinate_grid(H, W)),
 *                                mode='bilinear', padding_mode='reflection', align_corners=False): the sample is un-normalised as
 *                                ((g + 1) size - 1) / 2, reflected about -0.5 and size - 0.5 any number of times, clipped to
 *                                [0, size - 1]; a corner outside the map weighs nothing.  No grid tensor is written.  C 1..6, H and W
 *                                at least 2, B at most 65535; out must not be the frame.
 *   eamm_equi_tps_warp_points    coords [coords_batch,N,2] with coords_batch = 1 (one set for every image) or B -> out [B,N,2] and,
 *                                where jac is not NULL, jac [B,N,2,2] = d out / d coords = theta[b,i,j] + g_j,
 *                                g = sum_p w[b,p] U'(d_p) sign(c - c_p), sign(0) = 0 (autograd's abs).
 *   eamm_equi_tps_warp_points_backward  grad_out [B,N,2] and grad_jac [B,N,2,2] (each may be NULL, not both) -> grad_coords
 *                                [coords_batch,N,2], fully written: sum_i grad_out[i] jac[i][k] + sum_ij grad_jac[i][j] Hs[j][k],
 *                                Hs = sum_p w[b,p] U''(d_p) s s^T (the jacobian differentiated once more).  coords_batch = 1: the
 *                                images' terms are added in index order.
 * There is no gradient to the frame, theta or control_params: the reference draws the parameters and trains none of them.
 */
int eamm_equi_tps_warp_frame(int device, const float* frame, const float* theta, const float* control_params, int points, int B, int C,
                             int H, int W, float* out, void* stream);
int eamm_equi_tps_warp_points(int device, const float* coords, int coords_batch, const float* theta, const float* control_params, int points,
                              int B, int N, float* out, float* jac, void* stream);
int eamm_equi_tps_warp_points_backward(int device, const float* coords, int coords_batch, const float* theta, const float* control_params,
                                       int points, int B, int N, const float* grad_out, const float* grad_jac, float* grad_coords,
                                       void* stream);

/*
 * The optimiser step (the reference's torch.optim.Adam, train.py), a family of its own: eamm_optim_* (optim.hip).  Adam over a LIST of
 * fp32 tensors in as few launches as the list needs; per element, in torch's single-tensor order,
 *       g' = g + weight_decay p            (only when weight_decay != 0: L2 as torch.optim.Adam, not AdamW)
 *       m  = lerp(m, g', 1 - beta1)
 *       v  = beta2 v + (1 - beta2) g' g'
 *       p  = p - step_size m / (sqrt(v) / bc2_sqrt + eps)
 * with step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) PER TENSOR, computed by the caller (torch computes them
 * in Python floats) and handed over as fp32.
 *   eamm_optim_adam   p, g, m, v: HOST arrays of n device addresses, numel / step_size / bc2_sqrt: host arrays of n values.  Tensor i is
 *                     numel[i] contiguous floats at each of its four addresses; p, m and v are updated in place, g is only read.  The
 *                     addresses need 4-byte alignment only: a tensor whose four addresses are all 16-byte aligned is accessed four
 *                     floats at a time, any other one float at a time.  A tensor of length 0 is skipped (its addresses may be NULL).
 *                     The host arrays are copied into the launches' kernel arguments before the entry returns; it allocates nothing,
 *                     synchronises nothing and reads nothing back, and enqueues on `stream` only.  Refused by name: a NULL array, n < 0,
 *                     numel[i] outside 0 .. 2^36, a NULL or not 4-byte-aligned address of a tensor with elements, hyper-parameters that
 *                     are not finite, betas outside [0, 1), negative eps / weight_decay, bc2_sqrt[i] <= 0.  No two tensors may overlap.
 *   eamm_optim_adam_plan   HOST ONLY (touches no device): how eamm_optim_adam cuts a list of n lengths into launches, in list order.
 *                     Returns the number of launches (negative: an error) and fills, for the first max_launches of them,
 *                     launch_first / launch_count (tensors [first, first + count) of the list; count is at most the table capacity) and
 *                     launch_blocks (workgroups); elems_per_block[n] (may be NULL) gets per tensor the elements one workgroup covers, a
 *                     multiple of eamm_optim_adam_block_elems(), 0 for a length-0 tensor, which takes a table slot and no workgroup.
 *                     Tensor i is covered by ceil(numel[i] / elems_per_block[i]) workgroups, each element by exactly one.
 *   eamm_optim_adam_table_capacity   tensors per launch.   eamm_optim_adam_block_elems   E, the smallest elements-per-workgroup.
 */
int eamm_optim_adam(int device, int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel,
                    const float* step_size, const float* bc2_sqrt, double beta1, double beta2, double eps, double weight_decay,
                    void* stream);
int eamm_optim_adam_plan(int n, const long long* numel, int max_launches, int* launch_first, int* launch_count, int* launch_blocks,
                         long long* elems_per_block);
int eamm_optim_adam_table_capacity(void);
int eamm_optim_adam_block_elems(void);

#ifdef __cplusplus
}
#endif
#endif /* EAMM_HIP_H_ */
