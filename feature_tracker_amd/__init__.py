"""feature_tracker_amd — MI355X-native pyramidal KLT trackers, descriptor matchers (BRIEF Hamming, float cosine), Farneback dense flow
RAFT's correlation pyramid (all-pairs or on demand), convex flow upsampling, separable ConvGRU and whole update block, the warm start between video frames, KltVideoTracker (the sparse trackers over a frame sequence on a device-resident track table with masked Harris top-up), EpipolarRansac (two-view outlier rejection: RANSAC on the fundamental matrix, on the device), TwoViewRansac (the same with a homography as a second model and a rule that picks the model the data support), KeypointDecoder (a SuperPoint-style network's head tensors to keypoints, scores and descriptors on the device), SuperPoint (the network in front of it: its VGG with the max-pools fused into the convolutions, and the normalised dense descriptor map), MatchAssignment (LightGlue's assignment head: two descriptor sets to the log-assignment tensor, or without weights a dual-softmax matcher), TransformerLayer and LightGlue (LightGlue's self- and cross-attention layers, and the whole matcher from keypoints and descriptors to that tensor), NNFeatureMatcher's post-processing (mutual-best matching of those scores), and MatchVideoTracker (that pipeline over a frame sequence: a device-resident landmark table with a descriptor per slot, queried as the matcher's reference set and updated from its matches, so tracks keep their ids and return after up to max_lost hidden frames).

Product layout: ``csrc/`` (hand-written HIP kernels + the C ABI of ``include/ftk.h``),
``host/`` (C++ classes with the reference's names on top of the ABI), ``tracker.py`` (the same
interface for Python callers), ``dist.py`` (feature sharding across the GPUs of a node) and
``synth.py`` (deterministic synthetic workloads).  Importing the package does not load the
native library; the first compute call does, and fails loudly if it has not been built.
"""
from . import synth  # noqa: F401
from .epipolar import EpipolarRansac, EpipolarResult  # noqa: F401
from .keypoint_decoder import KeypointDecoder, KeypointResult  # noqa: F401
from .klt_video import KltVideoTracker  # noqa: F401
from .match_assignment import MatchAssignment  # noqa: F401
from .match_video import MatchVideoTracker  # noqa: F401
from .nn_matcher import NNFeatureMatcher, NNFeatureMatcherOptions  # noqa: F401
from .raft import ContextEncoder, CorrelationPyramid, FeatureEncoder, MotionEncoder, OnDemandCorrelation, Raft, RaftVideoTracker, SepConvGru, UpdateBlock, track_points_from_flow, upsample_flow, warm_start_flow  # noqa: F401
from .superpoint import SuperPoint  # noqa: F401
from .transformer import LightGlue, TransformerLayer, attention, rotary_encoding  # noqa: F401
from .two_view import TwoViewRansac, TwoViewResult  # noqa: F401
from .two_view_pose import TwoViewPose, TwoViewPoseResult  # noqa: F401
from .pnp import PnpRansac, PnpResult  # noqa: F401
from .track_odometry import TrackOdometry  # noqa: F401
from .tracker import (  # noqa: F401
    BriefDescriptor, BriefMatcher, CosineMatcher, DenseOpticalFlow, DenseOpticalFlowOptions, DirectMethod, DirectMethodOptions, DiskMatcher, SuperpointMatcher, Context, FeaturePointHarrisDetector, DescriptorMatcherOptions, ImagePyramid, OpticalFlow, OpticalFlowAffineKlt, OpticalFlowBasicKlt,
    OpticalFlowLssdKlt, OpticalFlowOptions, default_context, pack_brief, unpack_brief, refresh_env_switches,
    NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR,
)

__all__ = [
    "CorrelationPyramid", "OnDemandCorrelation", "MotionEncoder", "SepConvGru", "UpdateBlock", "upsample_flow", "track_points_from_flow", "warm_start_flow", "FeatureEncoder", "ContextEncoder", "Raft", "RaftVideoTracker", "KltVideoTracker", "MatchVideoTracker", "EpipolarRansac", "EpipolarResult", "TwoViewRansac", "TwoViewResult", "TwoViewPose", "TwoViewPoseResult", "PnpRansac", "PnpResult", "TrackOdometry", "KeypointDecoder", "KeypointResult", "SuperPoint", "MatchAssignment", "TransformerLayer", "LightGlue", "attention", "rotary_encoding", "NNFeatureMatcher", "NNFeatureMatcherOptions", "BriefDescriptor", "BriefMatcher", "CosineMatcher", "DenseOpticalFlow", "DenseOpticalFlowOptions", "DirectMethod", "DirectMethodOptions", "DiskMatcher", "SuperpointMatcher", "Context", "FeaturePointHarrisDetector", "DescriptorMatcherOptions", "ImagePyramid", "OpticalFlow", "OpticalFlowAffineKlt", "OpticalFlowBasicKlt",
    "OpticalFlowLssdKlt", "OpticalFlowOptions", "default_context", "pack_brief", "unpack_brief", "refresh_env_switches", "synth",
    "NOT_TRACKED", "TRACKED", "LARGE_RESIDUAL", "OUTSIDE", "NUMERIC_ERROR",
]
