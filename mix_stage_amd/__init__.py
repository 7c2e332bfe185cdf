"""mix_stage_amd -- MI355X-native (gfx950) implementation of the Mix-StAGE audio->pose conditional-mixture
GAN forward/backward path of chahuja/mix-stage, behind the reference's own nn.Module API.

The arithmetic lives in libmixstage_hip.so (hand-written HIP, C-ABI in include/mixstage.h); this package is
the host-side mirror of src/model/{layers,joint_late_cluster_soft_style,speech2gesture,gan}.py.
"""
from .layers import (AudioEncoder, ClusterClassify, ConvNormRelu, Curriculum, EmbLin, Group, PoseEncoder,  # noqa: F401
                     PoseStyleEncoder, TextEncoder1D, UNet1D, compute_dtype, freeze_batchnorm, frozen_batchnorm_blocks, number_dropout_sites,
                     set_compute_dtype, set_inference_folding)
from .ops import manual_dropout_seed  # noqa: F401
from .speech2gesture import Speech2Gesture_D  # noqa: F401
from .joint_late_cluster_soft_style import JointLateClusterSoftStyle4_D, JointLateClusterSoftStyle4_G  # noqa: F401
from .gan import GAN  # noqa: F401
from .lr_schedule import ConstantLR, ExponentialLR, as_lr_schedule  # noqa: F401
from .prestep import DevicePreStep  # noqa: F401
from .fit import DeviceColumnStats, DeviceKMeansFit  # noqa: F401
from .clip_store import DeviceClipStore, epoch_order, steps_per_epoch, window_table  # noqa: F401

__all__ = ['ConvNormRelu', 'UNet1D', 'AudioEncoder', 'PoseEncoder', 'PoseStyleEncoder', 'TextEncoder1D',
           'ClusterClassify', 'Group', 'EmbLin', 'Curriculum', 'JointLateClusterSoftStyle4_G',
           'JointLateClusterSoftStyle4_D', 'Speech2Gesture_D', 'GAN', 'set_compute_dtype', 'set_inference_folding',
           'compute_dtype', 'freeze_batchnorm', 'frozen_batchnorm_blocks', 'ExponentialLR', 'ConstantLR', 'as_lr_schedule',
           'number_dropout_sites', 'manual_dropout_seed', 'DevicePreStep', 'DeviceKMeansFit', 'DeviceColumnStats',
           'DeviceClipStore', 'window_table', 'epoch_order', 'steps_per_epoch']
