"""ctypes binding of libavhot.so (include/avhot.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device
is visible when a context is requested, this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libavhot.so")

c_i32p = C.POINTER(C.c_int32)
c_f64p = C.POINTER(C.c_double)
vp = C.c_void_p


class TrackerCfg(C.Structure):
    _fields_ = [("iou_threshold", C.c_double), ("max_age", C.c_int32), ("min_hits", C.c_int32),
                ("trajectory_length", C.c_int32)]


class KfCfg(C.Structure):
    _fields_ = [("dt", C.c_double), ("process_noise", C.c_double), ("measurement_noise", C.c_double)]


class StepSet(C.Structure):
    """av_step_set: the buffers one step of the one-launch step reads and writes."""
    _fields_ = [(k, C.c_void_p) for k in ("det_n", "det_box", "det_cls", "det_conf", "snap", "snap_n", "det2trk", "z", "vstate",
                                          "plan_state", "waypoints", "cost", "order")]


class StepLoop(C.Structure):
    """av_step_loop: what all steps of a loop share."""
    _fields_ = ([("tracker_cfg", TrackerCfg), ("kf_cfg", KfCfg)] +
                [(k, C.c_int32) for k in ("n_streams", "h", "w", "dcap", "tcap", "reserved")] +
                [(k, C.c_void_p) for k in ("frame_count", "det_status", "tracker_state", "kf_state")])


class PlannerCfg(C.Structure):
    _fields_ = [("planning_horizon", C.c_double), ("dt", C.c_double), ("num_samples", C.c_int32),
                ("reserved", C.c_int32), ("w_lateral", C.c_double), ("w_velocity", C.c_double),
                ("w_acceleration", C.c_double), ("w_curvature", C.c_double)]


class ObstacleCfg(C.Structure):
    """av_obstacle_cfg: image centre -> road plane (the BEV panel's constants) and the obstacle radius per class id."""
    _fields_ = [("x_center", C.c_double), ("x_scale", C.c_double), ("y_far", C.c_double), ("y_scale", C.c_double),
                ("radius", C.c_double * 16)]


class GroundCfg(C.Structure):
    """av_ground_cfg: one camera's ground-plane homography (image -> road), its inverse, the range limit and the box anchor."""
    _fields_ = [("g", C.c_double * 9), ("ginv", C.c_double * 9), ("max_range", C.c_double), ("anchor", C.c_int32),
                ("reserved", C.c_int32)]


class LensCfg(C.Structure):
    """av_lens_cfg: one camera's Brown-Conrady lens (raw intrinsics, k1 k2 p1 p2 k3, the rectified picture's intrinsics, size)."""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "nfx", "nfy", "ncx", "ncy")] + [
        ("w", C.c_int32), ("h", C.c_int32)]


class RigMount(C.Structure):
    """av_rig_mount: a camera's road frame in the vehicle's (cos and sin of the mount's yaw, the camera's ground point); 32 bytes."""
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("x", C.c_double), ("y", C.c_double)]


class RigCfg(C.Structure):
    """av_rig_cfg: av_rig_fuse's gate, max(merge_min, merge_scale * the larger radius); 16 bytes."""
    _fields_ = [("merge_scale", C.c_double), ("merge_min", C.c_double)]


class SurroundCfg(C.Structure):
    """av_surround_cfg: the surround panel's geometry (x_far metres at the top edge, m_per_px), blend (0 feather, 1 nearest) and the
    fill colour (b, g, r); 24 bytes."""
    _fields_ = [("x_far", C.c_double), ("m_per_px", C.c_double), ("blend", C.c_int32), ("fill", C.c_uint8 * 3), ("reserved", C.c_uint8)]


SURROUND_BLENDS = {"feather": 0, "nearest": 1}


class EgoflowCfg(C.Structure):
    """av_egoflow_cfg: the ground odometry's patch geometry, tile size T, search range R and the solver's settings; 64 bytes."""
    _fields_ = [("gh", C.c_int32), ("gw", C.c_int32), ("tile", C.c_int32), ("search", C.c_int32), ("f_far", C.c_double),
                ("m_per_px", C.c_double), ("frame_rate", C.c_double), ("min_texture", C.c_int32), ("gate_px", C.c_int32),
                ("inlier_px", C.c_double), ("min_inliers", C.c_int32), ("reserved", C.c_int32)]


EGOFLOW_ACCEPTED, EGOFLOW_LIVE, EGOFLOW_GATED, EGOFLOW_INLIER = 1, 2, 4, 8       # av_egoflow_tile.flags
EGOFLOW_TILE_FIELDS = [("flags", "<i4"), ("dy", "<i4"), ("dx", "<i4"), ("sad", "<i4"), ("texture", "<i4"), ("reserved", "<i4"),
                       ("sub_dy", "<f8"), ("sub_dx", "<f8"), ("f", "<f8"), ("l", "<f8")]                              # 56 bytes
EGOFLOW_TILE_BYTES = 56
EGOFLOW_MOTION_FIELDS = [("t_f", "<f8"), ("t_l", "<f8"), ("omega", "<f8"), ("rms", "<f8"), ("n_accepted", "<i4"), ("n_gated", "<i4"),
                         ("n_inliers", "<i4"), ("valid", "<i4"), ("vote_dy", "<i4"), ("vote_dx", "<i4"), ("reserved", "<i4", (2,))]
EGOFLOW_MOTION_BYTES = 64
EGOFLOW_STATE_FIELDS = [("x", "<f8"), ("y", "<f8"), ("psi", "<f8"), ("frames", "<i4"), ("reserved", "<i4")]          # 32 bytes
EGOFLOW_STATE_BYTES = 32
RIG_EGOFLOW_INFO_FIELDS = [("hypothesis", "<i4"), ("views", "<i4"), ("reserved", "<i4", (2,)), ("cam_accepted", "<i4", (8,)),
                           ("cam_gated", "<i4", (8,)), ("cam_inliers", "<i4", (8,)), ("cam_vote_dy", "<i4", (8,)),
                           ("cam_vote_dx", "<i4", (8,)), ("hyp_count", "<i4", (9,)), ("pad", "<i4")]      # av_rig_egoflow_info
RIG_EGOFLOW_INFO_BYTES = 216


class RoadmemCfg(C.Structure):
    """av_roadmem_cfg: the road memory's canvas (n cells a side, of m_per_px metres), max_age in frames, the surround panel's
    geometry (gh, gw, x_far, panel_m_per_px) and the fill colour (b, g, r); 48 bytes."""
    _fields_ = [("n", C.c_int32), ("max_age", C.c_int32), ("m_per_px", C.c_double), ("gh", C.c_int32), ("gw", C.c_int32),
                ("x_far", C.c_double), ("panel_m_per_px", C.c_double), ("fill", C.c_uint8 * 3), ("reserved", C.c_uint8 * 5)]


ROADMEM_STATE_FIELDS = [("i0", "<i4"), ("j0", "<i4"), ("frames", "<i4"), ("status", "<i4")]                          # 16 bytes
ROADMEM_STATE_BYTES = 16
ROADMEM_POSE_FIELDS = [("x", "<f8"), ("y", "<f8"), ("cs", "<f8"), ("sn", "<f8"), ("reset", "<i4"), ("reserved", "<i4")]   # 40 bytes
ROADMEM_POSE_BYTES = 40


class RoadLanesCfg(C.Structure):
    """av_road_lanes_cfg: the road-lane stage's row tests, votes, gate, lane widths, smoothing and path (metres); 144 bytes."""
    _fields_ = [(k, C.c_double) for k in ("min_len", "slope_max", "vote_len", "x_vote", "slope_tol", "y_max", "min_sep", "gate",
                                          "span_quad", "w_min", "w_max", "default_width", "alpha", "jump", "path_near", "path_far")] + [
        (k, C.c_int32) for k in ("min_votes", "max_coast", "one_sided", "n_points")]


ROAD_LANES_DEFAULTS = dict(min_len=0.5, slope_max=0.5, vote_len=0.25, x_vote=15.0, slope_tol=0.15, y_max=8.0, min_sep=2.0, gate=0.4,
                           span_quad=10.0, w_min=2.5, w_max=5.0, default_width=3.5, alpha=0.7, jump=1.0, path_near=2.0, path_far=40.0,
                           min_votes=16, max_coast=10, one_sided=1, n_points=50)
ROAD_LANES_MAX_BOUNDS, ROAD_LANES_MAX_SCAP = 8, 256
ROAD_BOUND_QUAD, ROAD_BOUND_KEPT, ROAD_BOUND_LEFT, ROAD_BOUND_RIGHT = 1, 2, 4, 8                      # av_road_lane_bound.flags
(ROAD_LANE, ROAD_ONE_SIDED, ROAD_COAST_LEFT, ROAD_COAST_RIGHT, ROAD_CHANGE_LEFT, ROAD_CHANGE_RIGHT,
 ROAD_NO_VOTER) = 1, 2, 4, 8, 16, 32, 64                                                               # av_road_lanes_row.status
ROAD_LANE_BOUND_FIELDS = [("a0", "<f8"), ("a1", "<f8"), ("a2", "<f8"), ("x_min", "<f8"), ("x_max", "<f8"), ("length", "<f8"),
                          ("n_members", "<i4"), ("views", "<i4"), ("flags", "<i4"), ("reserved", "<i4")]               # 64 bytes
ROAD_LANE_BOUND_BYTES = 64
ROAD_LANES_ROW_FIELDS = [("left", "<f8", (3,)), ("right", "<f8", (3,)), ("centre", "<f8", (3,)), ("width", "<f8"),
                         ("lane_offset", "<f8"), ("heading", "<f8"), ("curvature", "<f8"), ("n_bounds", "<i4"), ("lane_count", "<i4"),
                         ("lane_index", "<i4"), ("views", "<i4"), ("status", "<i4"), ("reserved", "<i4")]               # 128 bytes
ROAD_LANES_ROW_BYTES = 128
ROAD_LANES_INFO_FIELDS = [("cam_rows", "<i4", (8,)), ("n_over", "<i4"), ("n_off", "<i4"), ("n_short", "<i4"), ("n_steep", "<i4"),
                          ("n_voters", "<i4"), ("dir_bin", "<i4"), ("n_cand", "<i4"), ("n_peaks", "<i4"), ("m_star", "<f8")]  # 72 bytes
ROAD_LANES_INFO_BYTES = 72
ROAD_LANES_STATE_FIELDS = [("left", "<f8", (3,)), ("right", "<f8", (3,)), ("width", "<f8"), ("xmax_left", "<f8"), ("xmax_right", "<f8"),
                           ("has_left", "<i4"), ("has_right", "<i4"), ("miss_left", "<i4"), ("miss_right", "<i4"), ("has_width", "<i4"),
                           ("frames", "<i4")]                                                                         # 96 bytes
ROAD_LANES_STATE_BYTES = 96


class RoadMarksCfg(C.Structure):
    """av_road_marks_cfg: the road-mark stage's sample grid (metres), tap pattern, contrast, run thresholds (metres), colour rule and
    the frames a side's type is held and remembered; 88 bytes."""
    _fields_ = [(k, C.c_double) for k in ("x_near", "ds", "dl", "gap_solid", "gap_dash", "min_seen", "min_paint")] + [
        (k, C.c_int32) for k in ("n_samples", "core", "shoulder0", "shoulder1", "contrast", "yellow_tenths", "hold", "forget")]


ROAD_MARKS_DEFAULTS = dict(x_near=4.0, ds=0.1, dl=0.05, gap_solid=0.5, gap_dash=1.5, min_seen=8.0, min_paint=2.0, n_samples=210, core=5,
                           shoulder0=9, shoulder1=13, contrast=40, yellow_tenths=7, hold=3, forget=30)
ROAD_MARKS_MAX_SAMPLES = 512
ROAD_MARK_UNKNOWN, ROAD_MARK_SOLID, ROAD_MARK_DASHED = 0, 1, 2                                          # av_road_mark.type
ROAD_MARK_WHITE, ROAD_MARK_YELLOW = 1, 2                                                                # av_road_mark.colour
ROAD_MARK_AMBIGUOUS = 1                                                                                 # av_road_mark.flags
ROAD_MARK_TYPES, ROAD_MARK_COLOURS = ("unknown", "solid", "dashed"), ("none", "white", "yellow")
ROAD_MARK_FIELDS = [(k, "<i4") for k in ("type", "colour", "flags", "n_seen", "n_paint", "n_runs", "longest_gap", "n_gaps", "n_dashes",
                                         "contrast", "views", "reserved")] + [("dash_m", "<f8"), ("gap_m", "<f8")]   # 64 bytes
ROAD_MARK_BYTES = 64
ROAD_MARKS_SIDE_FIELDS = [(k, "<i4") for k in ("type", "colour", "observed", "observed_colour", "run", "bound")]  # 24 bytes
ROAD_MARKS_ROW_FIELDS = [("left", ROAD_MARKS_SIDE_FIELDS), ("right", ROAD_MARKS_SIDE_FIELDS), ("may_change_left", "<i4"),
                         ("may_change_right", "<i4"), ("reserved", "<i4", (2,))]                                    # 64 bytes
ROAD_MARKS_ROW_BYTES = 64
ROAD_MARKS_SIDE_STATE_FIELDS = [(k, "<i4") for k in ("type", "colour", "cand_type", "cand_colour", "run", "since")]  # 24 bytes
ROAD_MARKS_STATE_FIELDS = [("left", ROAD_MARKS_SIDE_STATE_FIELDS), ("right", ROAD_MARKS_SIDE_STATE_FIELDS), ("frames", "<i4"),
                           ("reserved", "<i4", (3,))]                                                               # 64 bytes
ROAD_MARKS_STATE_BYTES = 64
ROAD_MARKS_PROFILE_WORDS = 16                                                           # uint32 words per bit string: 512 samples


class LanePlanCfg(C.Structure):
    """av_lane_plan_cfg: the lane planner's vehicle half width and range (metres), the weights by mark type (unknown, solid, dashed)
    of crossing a line and of a waypoint on one, the weight of ending on one, and whether the lane's course is followed; 80 bytes."""
    _fields_ = [("half_width", C.c_double), ("x_far", C.c_double), ("w_cross", C.c_double * 3), ("w_on", C.c_double * 3),
                ("w_end", C.c_double), ("follow", C.c_int32), ("reserved", C.c_int32)]


LANEPLAN_DEFAULTS = dict(half_width=0.9, x_far=40.0, w_cross=(300.0, 1000.0, 0.0), w_on=(2.0, 5.0, 0.0), w_end=500.0, follow=1)
LANEPLAN_MAX_LINES, LANEPLAN_MAX_CAND, LANEPLAN_MAX_POINTS = 10, 192, 256
LANEPLAN_SRC_LEFT, LANEPLAN_SRC_RIGHT = 8, 9                                                          # av_lane_plan_line.source
LANEPLAN_KEEP, LANEPLAN_LEFT, LANEPLAN_RIGHT = 0, 1, 2                                               # av_lane_plan_row.maneuver
LANEPLAN_FOLLOW, LANEPLAN_CHANGED, LANEPLAN_FORCED, LANEPLAN_NO_LINES = 1, 2, 4, 8                  # av_lane_plan_row.flags
LANEPLAN_MANEUVERS = ("keep", "left", "right")
LANEPLAN_LINE_FIELDS = [("a0", "<f8"), ("a1", "<f8"), ("a2", "<f8"), ("xe", "<f8"), ("type", "<i4"), ("source", "<i4"),
                         ("reserved", "<i4", (2,))]                                                                  # 48 bytes
LANEPLAN_LINE_BYTES = 48
LANEPLAN_ROW_FIELDS = [("best", "<i4"), ("base_best", "<i4"), ("maneuver", "<i4"), ("delta", "<i4"), ("crossed", "<u4"),
                        ("crossed_solid", "<u4"), ("crossed_unknown", "<u4"), ("n_lines", "<i4"), ("flags", "<i4"), ("reserved", "<i4"),
                        ("base_cost", "<f8"), ("lane_cost", "<f8"), ("total", "<f8")]                                  # 64 bytes
LANEPLAN_ROW_BYTES = 64


class RigTrackCfg(C.Structure):
    """av_rig_track_cfg: the vehicle-frame tracker's filter, gate and life cycle (seconds, metres); 72 bytes."""
    _fields_ = [("dt", C.c_double), ("q_accel", C.c_double), ("r_meas", C.c_double), ("r_range", C.c_double), ("p0_pos", C.c_double),
                ("p0_vel", C.c_double), ("gate_scale", C.c_double), ("gate_min", C.c_double), ("max_age", C.c_int32),
                ("min_hits", C.c_int32)]


RIG_TRACK_HDR_BYTES = 64
RIG_TRACK_SLOT_BYTES = 96
RIG_TRACK_MAX = 512            # the largest tcap and ocap_in
RIG_TRACK_SLOT_FIELDS = [("id", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("age", "<i4"), ("views", "<i4"), ("views_ever", "<i4"),
                         ("reserved", "<i4", (2,)), ("x", "<f8", (4,)), ("p", "<f8", (3,)), ("r", "<f8")]           # 96 bytes


class RigInteractCfg(C.Structure):
    """av_rig_interact_cfg: the rig tagger's frame time, lane geometry (metres), passing speed, the tracker's min_hits and the
    class table of av_interaction_cfg; 112 bytes."""
    _fields_ = [("dt", C.c_double), ("corridor_half", C.c_double), ("adjacent_half", C.c_double), ("alongside", C.c_double),
                ("pass_speed", C.c_double), ("min_hits", C.c_int32), ("reserved", C.c_int32), ("class_kind", C.c_int32 * 16)]


RIG_INTERACT_HDR_BYTES = 16
RIG_INTERACT_SLOT_BYTES = 248
RIG_INTERACT_SLOT_FIELDS = [("id", "<i4"), ("cnt", "<i4"), ("lat", "<f8", (30,))]                                    # 248 bytes


class TrackFilterCfg(C.Structure):
    """av_track_filter_cfg: the per-track constant-velocity Kalman filter's noise and initial variances (px, frames)."""
    _fields_ = [("q_accel", C.c_double), ("r_meas", C.c_double), ("p0_pos", C.c_double), ("p0_vel", C.c_double)]


TRACK_FILTER_HDR_BYTES = 64
TRACK_FILTER_SLOT_FIELDS = [("id", "<i4"), ("reserved", "<i4"), ("x", "<f8", (4,)), ("p", "<f8", (3,))]     # 64 bytes


class LaneCfg(C.Structure):
    _fields_ = [("hough_threshold", C.c_int32), ("min_line_length", C.c_int32), ("max_line_gap", C.c_int32),
                ("max_segments", C.c_int32), ("smoothing_factor", C.c_double)]


# numpy structured dtype mirroring av_track_row (64 bytes)
TRACK_ROW_FIELDS = [("id", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("cls", "<i4"),
                    ("age", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("slot", "<i4"), ("hist_len", "<i4"),
                    ("flags", "<i4"), ("conf", "<f8"), ("vx", "<f4"), ("vy", "<f4")]
TRACK_ROW_BYTES = 64
TRACKER_HDR_BYTES = 64
KF_STATE_DOUBLES = 48
MANEUVER_STATE_DOUBLES = 32
MANEUVER_ROW_FIELDS = [("lateral", "<i4"), ("longitudinal", "<i4"), ("turning", "<i4"), ("reserved", "<i4"),
                       ("lateral_confidence", "<f8"), ("longitudinal_confidence", "<f8"), ("turning_confidence", "<f8"),
                       ("speed_kmh", "<f8"), ("acceleration", "<f8"), ("yaw_rate_deg", "<f8"), ("timestamp", "<f8")]
MANEUVER_ROW_BYTES = 72
INTERACTION_ROW_FIELDS = [("type", "<i4"), ("risk", "<i4"), ("agent_id", "<i4"), ("cls", "<i4"), ("confidence", "<f8"),
                          ("distance", "<f8"), ("relative_speed", "<f8"), ("ttc", "<f8")]
INTERACTION_ROW_BYTES = 48
INTERACTION_SUMMARY_FIELDS = [("agent_count", "<i4"), ("pedestrian_count", "<i4"), ("cyclist_count", "<i4"),
                              ("vehicle_count", "<i4"), ("n_interactions", "<i4"), ("primary_type", "<i4"),
                              ("overall_risk", "<i4"), ("primary_row", "<i4"), ("closest_distance", "<f8"),
                              ("min_ttc", "<f8"), ("timestamp", "<f8")]
INTERACTION_SUMMARY_BYTES = 56

SCENE_STATE_BYTES = 64
SCENE_ROW_FIELDS = [("gray_sum", "<u8"), ("green_count", "<u8"), ("lap_sum", "<i8"), ("lap_sumsq", "<u8"),
                    ("center_count", "<i4"), ("n_lines", "<i4"), ("avg_length", "<f8"), ("mean", "<f8"), ("green_ratio", "<f8"),
                    ("center_density", "<f8"), ("lap_var", "<f8"), ("scores", "<f8", (6,)), ("road_type_raw", "<i4"),
                    ("road_type", "<i4"), ("confidence", "<f8"), ("n_conditions", "<i4"), ("conditions", "<i4", (3,)),
                    ("condition_conf", "<f8", (3,)), ("lane_count", "<i4"), ("has_pedestrian", "<i4"), ("n_traffic", "<i4"),
                    ("overflow", "<i4"), ("timestamp", "<f8"), ("frame_count", "<i4"), ("history_len", "<i4"),
                    ("history", "<i4", (5,)), ("reserved", "<i4")]
SCENE_ROW_BYTES = 240
SCENE_CAT_TRAFFIC, SCENE_CAT_VEHICLE, SCENE_CAT_PEDESTRIAN = 1, 2, 4
TAGLOG_CHUNK = 1024
# av_lane_detect's `stages` bits and av_lane_workspace_view's view ids (AV_LANE_* of include/avhot.h)
LANE_KEEP_EDGES, LANE_PIXELS_ONLY, LANE_RESERVED, LANE_GENERIC_HOUGH = 1, 2, 4, 8
LANE_HOUGH_ONLY, LANE_FIT_ONLY, LANE_GIVEN_GRAY = 16, 32, 64
(LANE_VIEW_BLUR, LANE_VIEW_NMS, LANE_VIEW_EDGES, LANE_VIEW_MASKED, LANE_VIEW_THRESHOLDS, LANE_VIEW_SEGMENTS, LANE_VIEW_NSEG,
 LANE_VIEW_ACCUM, LANE_VIEW_HOUGH_PATH, LANE_VIEW_POINTS, LANE_VIEW_NPOINTS) = range(11)
TAGLOG_STATS_FIELDS = [("tag_count", "<i8", (64,)), ("n_frames", "<i8"), ("n_maneuver", "<i8"), ("risk_count", "<i8", (4,)),
                       ("speed_min", "<f8"), ("speed_max", "<f8"), ("speed_sum", "<f8")]
TAGLOG_STATS_BYTES = 584
TAGLOG_COLS_FIELDS = [("road_type_confidence", "<f8"), ("lateral_confidence", "<f8"), ("longitudinal_confidence", "<f8"),
                      ("turning_confidence", "<f8"), ("acceleration", "<f8"), ("yaw_rate_deg", "<f8"), ("min_ttc", "<f8"),
                      ("closest_distance", "<f8"), ("agent_count", "<i4"), ("pedestrian_count", "<i4"), ("cyclist_count", "<i4"),
                      ("vehicle_count", "<i4")]
TAGLOG_COLS_BYTES = 80


class TaglogWhere(C.Structure):
    """av_taglog_where (include/avhot.h): NaN = bound unset, a count bound <= 0 = none; 88 bytes."""
    _fields_ = ([(k, C.c_uint64) for k in ("all", "any", "none")] +
                [(k, C.c_double) for k in ("speed_min", "speed_max", "accel_min", "accel_max", "ttc_max", "distance_max")] +
                [(k, C.c_int32) for k in ("agents_min", "pedestrians_min", "cyclists_min", "vehicles_min")])


class BevCfg(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pixels_per_meter", C.c_double), ("x_min", C.c_double),
                ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double), ("n_candidates", C.c_int32),
                ("reserved", C.c_int32)]


class YoloSlice(C.Structure):
    """av_yolo_slice: `c` channels from channel `coff` of an NHWC map with `cstride` elements per pixel (test hook av_yolo_op)."""
    _fields_ = [("ptr", C.c_void_p)] + [(k, C.c_int32) for k in ("H", "W", "cstride", "coff", "c", "f32")]


class YoloOpInfo(C.Structure):
    """av_yolo_op_info: one op of the YOLO network as av_yolo_create built it (test hook av_yolo_op)."""
    _fields_ = ([(k, C.c_int32) for k in ("kind", "ksz", "stride", "act", "cin", "cout", "kpad", "kreal", "in_frame", "wgt_f32")]
                + [(k, YoloSlice) for k in ("in_", "in2", "out", "res")] + [("wgt", C.c_void_p), ("bias", C.c_void_p)])


YOLO_OP_CONV, YOLO_OP_STEM, YOLO_OP_POOLS, YOLO_OP_MAXPOOL, YOLO_OP_UPSAMPLE = range(5)


class YoloModel(C.Structure):
    """av_yolo_model: everything the YOLO graph builder reads (stage widths, C2f repeats, class count)."""
    _fields_ = [("ch", C.c_int32 * 5), ("rep", C.c_int32 * 4), ("neck_rep", C.c_int32), ("nc", C.c_int32), ("reserved", C.c_int32 * 5)]


class YoloStepInfo(C.Structure):
    """av_yolo_step_info: one launch of the YOLO forward's plan (test hook av_yolo_plan_step)."""
    _fields_ = ([(k, C.c_int32) for k in ("family", "first_op", "n_ops", "when")] + [("grid", C.c_int32 * 3), ("block", C.c_int32 * 3)]
                + [("lds_bytes", C.c_int32), ("lane", C.c_int32), ("variant", C.c_int32 * 6)])


(YOLO_K_MFMA, YOLO_K_GEMM128, YOLO_K_LDS, YOLO_K_WS3, YOLO_K_WS1, YOLO_K_GEMM_F32, YOLO_K_STEM_F32, YOLO_K_FIXED) = range(8)
YOLO_WHEN_ALWAYS, YOLO_WHEN_BGR_ALIGNED, YOLO_WHEN_BGR_UNALIGNED = range(3)


class JpegDesc(C.Structure):
    """av_jpeg_desc (include/avhot.h): one frame's headers as av_jpeg_parse reads them; 928 bytes."""
    _fields_ = ([(k, C.c_int32) for k in ("width", "height", "ncomp", "hs", "vs", "restart_interval", "n_segments", "flags", "scan_offset",
                                          "seg_base")] + [("byte_base", C.c_uint32), ("reserved", C.c_int32)] +
                [(k, C.c_uint8 * 4) for k in ("tq", "td", "ta", "pad")] + [("qt", C.c_uint8 * 64 * 4)] +
                [("dc_bits", C.c_uint8 * 16 * 2), ("dc_val", C.c_uint8 * 16 * 2), ("ac_bits", C.c_uint8 * 16 * 2), ("ac_val", C.c_uint8 * 256 * 2)])


JPEG_DESC_BYTES = 928
JPEG_SEG_FIELDS = [("begin", "<u4"), ("end", "<u4")]
JPEG_ECODE, JPEG_ERUN, JPEG_EBYTES, JPEG_ELEFT, JPEG_ESEGS, JPEG_EDESC = 1, 2, 4, 8, 16, 32
JPEG_EFULL, JPEG_HEADER_MAX = 64, 640              # av_jpeg_encode
JPEG_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
(EJPEG_TRUNCATED, EJPEG_FORMAT, EJPEG_SOF, EJPEG_ARITH, EJPEG_PRECISION, EJPEG_COMPONENTS, EJPEG_SAMPLING, EJPEG_DQT16, EJPEG_MULTISCAN,
 EJPEG_SIZE, EJPEG_TABLE, EJPEG_SCAN, EJPEG_SEGCAP) = range(-101, -114, -1)


class InteractionCfg(C.Structure):
    _fields_ = [("frame_h", C.c_int32), ("frame_w", C.c_int32), ("class_kind", C.c_int32 * 16)]
PRIM_FIELDS = [("type", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"),
               ("x3", "<i4"), ("y3", "<i4"), ("p", "<i4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("reserved", "<i4")]
PRIM_BYTES = 48
PRIM_RECT, PRIM_SEG, PRIM_QUAD, PRIM_DISC, PRIM_RING, PRIM_GLYPH, PRIM_BLEND_RECT, PRIM_POLY_BLEND = 1, 2, 3, 4, 5, 6, 7, 8
VSTATE_DOUBLES = 12
NAME_BYTES = 24
VIEW_DETECTIONS, VIEW_LANES, VIEW_TRACKS, VIEW_INFO, VIEW_SUMMARY, VIEW_GAUGE, VIEW_DEMO, VIEW_ALL = 1, 2, 4, 8, 16, 32, 31, 63


class CamviewArgs(C.Structure):
    """av_camview_args (include/avhot.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_streams", "h", "w", "flags", "n_frames", "frame", "max_det", "tcap", "trajectory_length",
                                         "max_name", "n_det_names", "n_det_colors", "n_trk_names", "reserved")] + [("fps", C.c_double)] + [
        (n, C.c_void_p) for n in ("det_n", "det_box", "det_conf", "det_cls", "det_names", "det_name_len", "det_colors", "lane_pts",
                                  "lane_info", "snap", "snap_n", "tracker_state", "trk_names", "trk_name_len", "vstate")]


def name_table(names, what="class names"):
    """{id: name} or a name list -> (uint8 [n][NAME_BYTES], int32 lengths [n], -1 where there is no such id): the device tables of
    av_camview_build.  A name of more than NAME_BYTES - 1 characters, or one outside Latin-1, raises ValueError."""
    import numpy as np
    items = names.items() if isinstance(names, dict) else enumerate(names)
    items = [(int(k), str(v)) for k, v in items]
    n = max([k for k, _ in items if k >= 0], default=-1) + 1
    tab, lens = np.zeros((max(n, 1), NAME_BYTES), np.uint8), np.full(max(n, 1), -1, np.int32)
    for k, v in items:
        if k < 0:
            continue
        try:
            raw = v.encode("latin-1")
        except UnicodeEncodeError:
            raise ValueError("%s: %r has characters outside Latin-1" % (what, v)) from None
        if len(raw) > NAME_BYTES - 1:
            raise ValueError("%s: %r is longer than %d characters" % (what, v, NAME_BYTES - 1))
        tab[k, :len(raw)] = np.frombuffer(raw, np.uint8)
        lens[k] = len(raw)
    return tab, lens
WP_DOUBLES = 6

# (name, restype, argtypes); everything returns int status except the three noted
_SIGS = [
    ("av_version", C.c_int, []),
    ("av_last_error_string", C.c_char_p, []),
    ("av_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("av_ctx_create", C.c_int, [C.c_int, C.POINTER(vp)]),
    ("av_ctx_destroy", C.c_int, [vp]),
    ("av_ctx_device", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("av_side_stream", C.c_int, [vp, C.POINTER(vp)]),
    ("av_fork", C.c_int, [vp, vp]),
    ("av_join", C.c_int, [vp, vp]),
    ("av_graph_begin", C.c_int, [vp, vp]),
    ("av_graph_end", C.c_int, [vp, vp, C.POINTER(C.c_int)]),
    ("av_graph_launch", C.c_int, [vp, C.c_int, vp]),
    ("av_graph_destroy", C.c_int, [vp, C.c_int]),
    ("av_event_create", C.c_int, [C.POINTER(vp)]),
    ("av_event_destroy", C.c_int, [vp]),
    ("av_event_record", C.c_int, [vp, vp]),
    ("av_event_elapsed_ms", C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    ("av_stream_sync", C.c_int, [vp]),
    ("av_stream_sync_spin", C.c_int, [vp]),
    ("av_host_alloc", C.c_int, [C.POINTER(vp), C.c_size_t]),
    ("av_host_free", C.c_int, [vp]),
    ("av_copy_h2d", C.c_int, [vp, vp, C.c_size_t, vp]),
    ("av_copy_d2h", C.c_int, [vp, vp, C.c_size_t, vp, C.c_int]),
    ("av_simdet_generate", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    ("av_tracker_state_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("av_tracker_reset", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    ("av_tracker_update", C.c_int, [vp, vp, C.POINTER(TrackerCfg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp,
                                    C.c_int, vp, vp, vp, vp]),
    ("av_wire_table_bytes", C.c_size_t, [C.c_int]),
    ("av_pack_tracks", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    ("av_comm_unique_id", C.c_int, [vp]),
    ("av_comm_create", C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
    ("av_comm_destroy", C.c_int, [vp]),
    ("av_allgather_tracks", C.c_int, [vp, vp, vp, vp, vp, C.c_size_t]),
    ("av_kf_reset", C.c_int, [vp, vp, C.c_int, vp]),
    ("av_kf_step", C.c_int, [vp, vp, C.POINTER(KfCfg), C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    ("av_planner_configure", C.c_int, [vp, C.POINTER(PlannerCfg)]),
    ("av_planner_dims", C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("av_planner_launch_shape", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_i32p]),
    ("av_planner_plan", C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]),
    ("av_planner_plan_each", C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
    ("av_track_obstacles", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]),
    ("av_planner_plan_moving", C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
    ("av_track_obstacles_moving", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), C.c_double, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp,
                                            vp]),
    ("av_track_filter_state_bytes", C.c_size_t, [C.c_int]),
    ("av_track_filter_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_track_filter_update", C.c_int, [vp, vp, C.POINTER(TrackFilterCfg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    ("av_track_obstacles_filtered", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), C.c_double, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int,
                                              vp, vp]),
    ("av_dets_to_tracker", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    ("av_lane_paths", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int,
                                C.c_int, vp, vp, vp]),
    ("av_ground_make", C.c_int, [c_f64p, C.c_double, C.c_int, C.POINTER(GroundCfg)]),
    ("av_track_obstacles_ground", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp,
                                            vp, vp, vp, C.c_int, vp, vp, vp]),
    ("av_lane_paths_ground", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp,
                                       vp]),
    ("av_ground_warp", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double,
                                 C.POINTER(C.c_uint8), vp]),
    ("av_lens_make", C.c_int, [c_f64p, c_f64p, c_f64p, C.c_int, C.c_int, C.POINTER(LensCfg)]),
    ("av_lens_map_rectify", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    ("av_lens_map_ground", C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp]),
    ("av_remap", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_uint8), vp]),
    ("av_track_obstacles_ground_lens", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), vp, vp, C.c_int, C.c_int, C.c_double, C.c_int,
                                                 C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp]),
    ("av_track_obstacles_ground_cls", C.c_int, [vp, vp, C.POINTER(ObstacleCfg), vp, vp, C.c_int, C.c_int, C.c_double, C.c_int,
                                                C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]),
    ("av_rig_fuse_cls", C.c_int, [vp, vp, C.POINTER(RigCfg), C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp,
                                  vp, vp, vp]),
    ("av_rig_track_cls", C.c_int, [vp, vp, C.POINTER(RigTrackCfg), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int,
                                   vp, vp, vp, vp, vp, vp, vp]),
    ("av_rig_interact_state_bytes", C.c_size_t, [C.c_int]),
    ("av_rig_interact_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_rig_interact", C.c_int, [vp, vp, C.POINTER(RigInteractCfg), C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    ("av_tags_pack_slots", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]),
    ("av_rig_fuse", C.c_int, [vp, vp, C.POINTER(RigCfg), C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp,
                              vp]),
    ("av_rig_track_state_bytes", C.c_size_t, [C.c_int]),
    ("av_rig_track_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_rig_track", C.c_int, [vp, vp, C.POINTER(RigTrackCfg), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp,
                               vp, vp, vp, vp]),
    ("av_rig_surround", C.c_int, [vp, vp, C.POINTER(SurroundCfg), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp,
                                  vp]),
    ("av_rig_view_prim_cap", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("av_rig_view_build", C.c_int, [vp, vp, C.POINTER(SurroundCfg), C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int,
                                    vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    ("av_hot_step", C.c_int, [vp, vp, C.POINTER(StepLoop), C.POINTER(StepSet), vp, C.c_int, C.c_int]),
    ("av_hot_step_fits", C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_hot_step_plan", C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_size_t)]),
    ("av_hot_step_seq", C.c_int, [vp, vp, C.POINTER(StepLoop), C.POINTER(StepSet), vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
    ("av_hot_steps_seq", C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(StepLoop), C.POINTER(StepSet), vp, vp, C.c_int, C.c_int, vp,
                                   C.c_int, C.c_int]),
    ("av_planner_generate", C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp]),
    ("av_planner_evaluate", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]),
    ("av_planner_evaluate_moving", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]),
    ("av_lane_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_lane_workspace_init", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    ("av_lane_workspace_view", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t)]),
    ("av_raster_draw", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int]),
    ("av_bev_prim_cap", C.c_int, [vp, C.c_int, C.c_int]),
    ("av_bev_build", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    ("av_i420_to_bgr", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    ("av_resize_into", C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_raster_draw_to", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int]),
    ("av_camview_prim_cap", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_camview_build", C.c_int, [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]),
    ("av_view_compose_size", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    ("av_view_compose", C.c_int, [vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_char_p, C.c_char_p]),
    ("av_format_fixed", C.c_int, [C.c_double, C.c_int, vp, C.c_int]),
    ("av_bgr_to_i420", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    ("av_jpeg_parse", C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]),
    ("av_jpeg_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("av_jpeg_decode", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp]),
    ("av_jpeg_encode_header", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    ("av_jpeg_encode_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_jpeg_encode", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp]),
    ("av_synth_frames", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    ("av_maneuver_reset", C.c_int, [vp, vp, C.c_int, vp]),
    ("av_interaction_state_bytes", C.c_size_t, [C.c_int]),
    ("av_interaction_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_interaction_detect", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("av_maneuver_detect", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    ("av_yolo_param_count", C.c_size_t, []),
    ("av_yolo_create", C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(vp)]),
    ("av_yolo_create_ex", C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(vp)]),
    ("av_yolo_model_preset", C.c_int, [C.c_int, C.c_int, C.POINTER(YoloModel)]),
    ("av_yolo_model_param_count", C.c_size_t, [C.POINTER(YoloModel)]),
    ("av_yolo_create_model", C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(YoloModel), vp, C.c_size_t, C.c_int, C.POINTER(vp)]),
    ("av_yolo_model_of", C.c_int, [vp, C.POINTER(YoloModel)]),
    ("av_yolo_destroy", C.c_int, [vp]),
    ("av_yolo_dims", C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("av_yolo_forward", C.c_int, [vp, vp, vp, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp]),
    ("av_yolo_keep_logits", C.c_int, [vp, C.c_int]),
    ("av_yolo_defer_tail", C.c_int, [vp, C.c_int]),
    ("av_yolo_join_tail", C.c_int, [vp, vp]),
    ("av_yolo_tensor", C.c_int, [vp, C.c_int, C.POINTER(vp)] + [C.POINTER(C.c_int)] * 5),
    ("av_yolo_tail", C.c_int, [vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp]),
    ("av_yolo_op_count", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("av_yolo_op", C.c_int, [vp, C.c_int, C.POINTER(YoloOpInfo)]),
    ("av_yolo_plan_count", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("av_yolo_plan_step", C.c_int, [vp, C.c_int, C.POINTER(YoloStepInfo)]),
    ("av_lane_detect", C.c_int, [vp, vp, C.POINTER(LaneCfg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                 vp, C.c_int]),
    ("av_scene_state_bytes", C.c_size_t, [C.c_int]),
    ("av_scene_reset", C.c_int, [vp, vp, C.c_int, vp]),
    ("av_scene_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("av_scene_workspace_init", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    ("av_scene_classify", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp,
                                    vp, vp, vp, vp]),
    ("av_tags_pack", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]),
    ("av_taglog_append", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]),
    ("av_taglog_workspace_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("av_taglog_search", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp,
                                   C.c_int, vp, vp]),
    ("av_taglog_segments", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                     C.c_int, vp, C.c_int, vp, vp]),
    ("av_taglog_stats", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    ("av_tags_cols", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    ("av_taglog_append_ex", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
    ("av_taglog_search_where", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(TaglogWhere), C.c_int, C.c_int, vp,
                                         C.c_int, vp, vp]),
    ("av_taglog_segments_where", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(TaglogWhere), C.c_int, C.c_int,
                                           C.c_int, vp, C.c_int, vp, vp]),
    ("av_taglog_gather", C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]),
    ("av_egoflow_tiles", C.c_int, [C.POINTER(EgoflowCfg), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("av_egoflow_patch", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    ("av_egoflow_match", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), C.c_int, vp, vp, vp, vp]),
    ("av_egoflow_solve", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), C.c_int, vp, vp]),
    ("av_egoflow_measure", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), C.c_int, vp, vp, vp, vp]),
    ("av_egoflow_update", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("av_rig_egoflow_solve", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), C.c_int, C.c_int, vp, vp, vp, vp]),
    ("av_rig_egoflow_update", C.c_int, [vp, vp, C.POINTER(EgoflowCfg), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp]),
    ("av_roadmem_check", C.c_int, [C.POINTER(RoadmemCfg)]),
    ("av_roadmem_pose_from", C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    ("av_roadmem_update", C.c_int, [vp, vp, C.POINTER(RoadmemCfg), C.c_int, vp, vp, vp, vp, vp, vp]),
    ("av_roadmem_fill", C.c_int, [vp, vp, C.POINTER(RoadmemCfg), C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    ("av_roadmem_step", C.c_int, [vp, vp, C.POINTER(RoadmemCfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("av_roadmem_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_road_lanes_check", C.c_int, [C.POINTER(RoadLanesCfg)]),
    ("av_road_lanes_state_bytes", C.c_size_t, []),
    ("av_road_lanes", C.c_int, [vp, vp, C.POINTER(RoadLanesCfg), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                vp, C.c_int, vp, vp, vp]),
    ("av_road_lanes_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_road_marks_check", C.c_int, [C.POINTER(RoadMarksCfg)]),
    ("av_road_marks_state_bytes", C.c_size_t, []),
    ("av_road_marks", C.c_int, [vp, vp, C.POINTER(RoadMarksCfg), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    ("av_road_marks_reset", C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    ("av_lane_plan_check", C.c_int, [C.POINTER(LanePlanCfg)]),
    ("av_lane_plan", C.c_int, [vp, vp, C.POINTER(LanePlanCfg), C.c_int, C.c_int, C.c_int] + [vp] * 14),
]

# entry points added by later translation units; bound when present in the header list below
_OPTIONAL_SIGS = []

_lib = None


def declared_symbols():
    """Every function name include/avhot.h declares (parsed from the header text)."""
    import re

    hdr = os.path.join(os.path.dirname(_HERE), "include", "avhot.h")
    txt = open(hdr).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(av_[a-z0-9_]+)\s*\(", txt)))


def _preload_hip_runtime():
    """One HIP runtime per process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7).  libavhot.so
    NEEDs libamdhip64.so.7 too; if the system copy under /opt/rocm were mapped first, torch would
    later map its bundled copy as a second runtime, and the two do not share devices, streams or
    allocations.  Mapping torch's copy first makes the dynamic loader satisfy our NEEDED entry
    with it (SONAME match).
    """
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def lib():
    """The loaded library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libavhot.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "-- this package has no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, res, args in _SIGS + _OPTIONAL_SIGS:
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def register(sigs):
    """Used by lane/yolo bindings to add their signatures before first use."""
    global _lib
    _OPTIONAL_SIGS.extend(sigs)
    if _lib is not None:
        for name, res, args in sigs:
            fn = getattr(_lib, name)
            fn.restype = res
            fn.argtypes = args


def step_flag_ints(n_streams):
    """AV_STEP_FLAG_INTS(n_streams) of include/avhot.h: int32 words of the overlapped steps' sequence flags."""
    return 65 * n_streams + (n_streams & 1) + 32 + 64


def step_plan(ctx_handle, n_streams, dcap, tcap, depth):
    """av_hot_step_plan: (rc, waves per workgroup, workgroups per CU from the occupancy query -- 0 at depth 1 --, dynamic LDS bytes) of
    the one-launch step with `depth` launches in flight; rc != 0 (see av_last_error_string) where no shape fits."""
    w, p, b = C.c_int(), C.c_int(), C.c_size_t()
    rc = lib().av_hot_step_plan(ctx_handle, n_streams, dcap, tcap, depth, C.byref(w), C.byref(p), C.byref(b))
    return rc, w.value, p.value, b.value


def step_i32(v):
    """A step number (kept modulo 2^32) as the signed int the C ABI takes."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def check(rc):
    if rc != 0:
        raise RuntimeError("libavhot: %s (code %d)" % (lib().av_last_error_string().decode(), rc))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


class Context:
    """Owns one av_ctx on one device."""

    def __init__(self, device=0):
        L = lib()
        h = vp()
        check(L.av_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)
        s = vp()
        check(L.av_side_stream(h, C.byref(s)))
        self.side_stream = s

    def close(self):
        if getattr(self, "handle", None):
            lib().av_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    """Process-wide context per device (the per-frame drop-in classes share it)."""
    c = _default_ctx.get(device)
    if c is None or c.handle is None:
        c = Context(device)
        _default_ctx[device] = c
    return c


def stream_handle(stream=None):
    """hipStream_t of a torch stream (default: torch's current stream) as c_void_p."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)
