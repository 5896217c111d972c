"""closed_chain_motion_planner_amd — MI355X-native batched closed-chain constraint projector.

Only the projector hot path of jkw0701/closed_chain_motion_planner: the C-ABI library
`libccmp.so` (include/ccmp.h, csrc/) and this thin host mirror of the reference's constraint
interface.  Importing the package needs neither a GPU nor the built library; using it does.
"""
from ._lib import CCMP_JAC_ANALYTIC, CCMP_JAC_FD, CcmpError, CcmpProblem, describe, get_option, option_table  # noqa: F401
from .constraint import ArmModel, Communicator, Context, KinematicChainConstraint, load_config  # noqa: F401

from .space import (check_motion, format_graphml, format_graphviz, format_path_matrix, geodesic_interpolate,  # noqa: F401
                    jy_ProjectedStateSampler, jy_ProjectedStateSpace, next_sampler_seed, parse_graphml, parse_path_matrix,
                    splitmix64)

from .scene import ProxyScene, ProxyValidityChecker, default_allowed, skeleton_spheres  # noqa: F401

from .roadmap import PLAN_STATUS, Plan, plan_check_ref, plan_connected_ref, plan_options, plan_prefix_ref  # noqa: F401
from .roadmap import RRTC_STATUS, RRTConnect, nearest_in_tree_ref, rrtc_connected_ref, rrtc_nearest_shape, rrtc_options, rrtc_pick, rrtc_pick_ref  # noqa: F401
from .roadmap import Roadmap, closest_ref, commit_ref, graph_labels_ref, joint_distance, pose_distance, pose_from_t_wo, shortest_paths_ref  # noqa: F401

from .dense import DENSE_DISTINCT, dense_arc_ref, dense_layout_ref  # noqa: F401

from .shortcut import SHORTCUT_MAX_LEN, shortcut_pairs_ref, shortcut_select, shortcut_select_ref  # noqa: F401

from .smooth import SMOOTH_STATS, SMOOTH_STOP, smooth_len_after, smooth_mid_ref  # noqa: F401

from .retime import (PANDA_ACCELERATION_LIMITS, PANDA_JERK_LIMITS, PANDA_VELOCITY_LIMITS, RETIME_STATUS, SAMPLE_KINDS, arc_bracket_ref, resample_targets_ref,  # noqa: F401
                     timestamps_ref)

from .setpoints import SETPOINT_PEAKS, SETPOINT_STATUS, setpoint_tangents_ref, setpoints_ref  # noqa: F401

from .fit import FIT_STATUS, fit_timestamps_ref  # noqa: F401

from .jerk import JERK_PEAKS, JERK_STATUS, jerk_next_window_ref, jerk_setpoints_ref  # noqa: F401

from .ik import ik_options, pose_ik_ref, pose_ik_vetted_ref  # noqa: F401

from .object import ObjectChecker, object_propose_ref, object_valid_ref, pose_interpolate  # noqa: F401

__version__ = "0.6.0"
