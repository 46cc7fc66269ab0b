"""eamm_amd -- MI355X (gfx950) implementation of EAMM's dense-motion + OcclusionAwareGenerator path.

Python host code (this package) mirrors the reference's module interface for the path and drives
libeamm_hip.so, a C-ABI library of hand-written HIP kernels (include/eamm_hip.h).  See DESIGN.md.
"""
from .config import hot_path_config, tiny_config  # noqa: F401
from .generator import OcclusionAwareGenerator  # noqa: F401
from .engine import Engine  # noqa: F401
from .clip import EngineBackend, animate_clip, driving_keypoints, shard_bounds  # noqa: F401
from .keypoints import apply_emotion_offsets, normalize_kp, one_euro_smooth, smooth_keypoints  # noqa: F401
from .pipeline import animate_from_features  # noqa: F401
from .keypoint_detector import KPDetector, KPDetector_a  # noqa: F401
from .emotion_detector import EmotionDetector  # noqa: F401
from .audio_feature import AudioFeatureNet  # noqa: F401
from .audio_input import animate_from_audio, mfcc, mfcc_reference, mfcc_windows, prepare_pose, read_wav  # noqa: F401
from .video_input import (EmotionVideo, align_video, crop_source, crop_source_reference, draw_augmentation,  # noqa: F401
                          emotion_video_reference, perspective_params, similarity_transform)
from .deconv_tail import DeconvTail, SplitFeatureMap  # noqa: F401
from .sync_batchnorm import SynchronizedBatchNorm2d  # noqa: F401
from .data_parallel import all_reduce_gradients  # noqa: F401
from .perceptual import ImagePyramide, PerceptualLoss, Vgg19  # noqa: F401
from .perceptual_ops import frozen_conv3x3, l1_pair, pyramid_levels, relu_pool, vgg_input  # noqa: F401
from .discriminator import Discriminator, MultiScaleDiscriminator  # noqa: F401
from .disc_ops import conv4_valid, norm_act_pool  # noqa: F401
from .gan_loss import discriminator_gan_loss, generator_gan_loss  # noqa: F401
from .equivariance import Transform, equivariance_loss  # noqa: F401
from .equivariance_ops import tps_warp_frame, tps_warp_points  # noqa: F401
from .optim import Adam  # noqa: F401
from .optim_ops import adam_step  # noqa: F401
from .config import kp_detector_config, kp_detector_a_config, tiny_kp_config, emotion_detector_config, emotion_augmentation_config  # noqa: F401

__all__ = ["OcclusionAwareGenerator", "Engine", "EngineBackend", "animate_clip", "animate_from_features", "animate_from_audio", "mfcc", "mfcc_reference", "mfcc_windows", "prepare_pose", "read_wav", "EmotionVideo", "align_video", "crop_source", "crop_source_reference", "draw_augmentation", "emotion_video_reference", "perspective_params", "similarity_transform", "emotion_augmentation_config", "driving_keypoints", "shard_bounds", "normalize_kp", "apply_emotion_offsets", "smooth_keypoints", "one_euro_smooth", "KPDetector", "KPDetector_a", "EmotionDetector", "AudioFeatureNet", "DeconvTail", "SplitFeatureMap", "SynchronizedBatchNorm2d",
           "Vgg19", "ImagePyramide", "PerceptualLoss", "vgg_input", "pyramid_levels", "relu_pool", "l1_pair", "frozen_conv3x3",
           "Discriminator", "MultiScaleDiscriminator", "conv4_valid", "norm_act_pool", "generator_gan_loss", "discriminator_gan_loss",
           "Transform", "equivariance_loss", "tps_warp_frame", "tps_warp_points",
           "Adam", "adam_step",
           "all_reduce_gradients", "hot_path_config", "tiny_config"]
