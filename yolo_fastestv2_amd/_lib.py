"""ctypes binding of libyfv2.so (the C ABI declared in include/yfv2.h).

There is deliberately NO fallback: if the shared library is missing or does not
export the ABI this module raises, and every product entry point fails loudly.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or
``make -C yolo_fastestv2_amd/csrc``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# YFV2_LIB: opt-in override used only for same-box A/B of two builds (tools/gpu_quick.sh)
LIB_PATH = os.environ.get("YFV2_LIB") or os.path.join(_HERE, "libyfv2.so")
ABI_VERSION = 7
MAX_DET = 300

OK, ERR_ARG, ERR_CONFIG, ERR_DEVICE, ERR_WEIGHTS, ERR_STATE, ERR_BATCH, ERR_RANGE = 0, -1, -2, -3, -4, -5, -6, -7


class Config(C.Structure):
    _fields_ = [("classes", C.c_int32), ("anchor_num", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("anchors", C.c_double * 12), ("max_batch", C.c_int32), ("device", C.c_int32)]


class Plan(C.Structure):
    """yfv2_plan (include/yfv2.h): WHICH kernels compute the path.  All zero = the default plan."""
    _fields_ = [("struct_size", C.c_int32), ("fp32_matrix", C.c_int32), ("layer_by_layer", C.c_int32), ("post_two_launches", C.c_int32),
                ("front_two_launches", C.c_int32), ("towers_unpaired", C.c_int32), ("lanes", C.c_int32), ("trace", C.c_int32), ("trace_step", C.c_int32)]


PLAN_FIELDS = ("fp32_matrix", "layer_by_layer", "post_two_launches", "front_two_launches", "towers_unpaired", "lanes", "trace", "trace_step")


def make_plan(plan=None):
    """dict (or None) -> Plan.  Unknown keys are an error: a misspelt switch must not silently select the default plan."""
    p = Plan()
    p.struct_size = C.sizeof(Plan)
    p.trace_step = -1
    for k, v in (plan or {}).items():
        if k not in PLAN_FIELDS:
            raise ValueError("unknown plan switch %r (known: %s)" % (k, ", ".join(PLAN_FIELDS)))
        setattr(p, k, int(v))
    return p


def plan_from_env(env=None):
    """The plan the measurement tools and the fallback-plan tests ask for through THEIR environment (the library itself reads none):
    YFV2_BF6=0 -> fp32_matrix, YFV2_FUSED=0 -> layer_by_layer, YFV2_POSTFUSE=0 -> post_two_launches, YFV2_FRONT=0 -> front_two_launches,
    YFV2_TPAIR=0 -> towers_unpaired, YFV2_LANES=N -> lanes, YFV2_TRACE=1 [YFV2_TRACE_STEP=k] -> trace [trace_step]."""
    env = os.environ if env is None else env
    off = lambda k: 1 if env.get(k, "1")[:1] == "0" else 0
    plan = {"fp32_matrix": off("YFV2_BF6"), "layer_by_layer": off("YFV2_FUSED"), "post_two_launches": off("YFV2_POSTFUSE"),
            "front_two_launches": off("YFV2_FRONT"), "towers_unpaired": off("YFV2_TPAIR")}
    if env.get("YFV2_LANES"):
        plan["lanes"] = int(env["YFV2_LANES"])
    if env.get("YFV2_TRACE", "")[:1] == "1":
        plan["trace"] = 1
        if env.get("YFV2_TRACE_STEP"):
            plan["trace_step"] = int(env["YFV2_TRACE_STEP"])
    return plan


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


class SgdItem(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("momentum_buf", C.c_void_p), ("n", C.c_int64), ("first_step", C.c_int32), ("reserved", C.c_int32)]


class Frame(C.Structure):
    """yfv2_frame (include/yfv2.h): one uint8 HWC frame of a ragged batch; data is a DEVICE pointer."""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("row_pitch", C.c_int64)]


class FrameYuv(C.Structure):
    """yfv2_frame_yuv (include/yfv2.h): one YUV 4:2:0 frame of a ragged batch, planes read in place; y, u, v are DEVICE pointers."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("pitch_y", C.c_int64), ("pitch_c", C.c_int64),
                ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32), ("colour", C.c_int32)]


class Tile(C.Structure):
    """yfv2_tile (include/yfv2.h): a rectangle inside frames[frame]."""
    _fields_ = [("frame", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class CropRule(C.Structure):
    """yfv2_crop_rule (include/yfv2.h): the size, pad, cut and class filter of second-stage crops; classes is a HOST pointer."""
    _fields_ = [("out_h", C.c_int32), ("out_w", C.c_int32), ("pad_x", C.c_float), ("pad_y", C.c_float), ("max_per_frame", C.c_int32),
                ("classes", C.POINTER(C.c_int32)), ("n_classes", C.c_int32)]


class CropTensor(C.Structure):
    """yfv2_crop_tensor (include/yfv2.h): dtype, plane order, mean / std, letterbox and fill of crops written as a network's input."""
    _fields_ = [("dtype", C.c_int32), ("rgb", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("letterbox", C.c_int32),
                ("fill", C.c_uint8 * 3)]


F32, F16 = 0, 1


class TrackRule(C.Structure):
    """yfv2_track_rule (include/yfv2.h): the parameters of the per-stream IoU tracker."""
    _fields_ = [("max_tracks", C.c_int32), ("match_thres", C.c_double), ("class_aware", C.c_int32), ("init_conf", C.c_float),
                ("max_misses", C.c_int32), ("confirm_hits", C.c_int32)]


class TrackMotion(C.Structure):
    """yfv2_track_motion (include/yfv2.h): the noise scales of the tracker's constant-velocity filters."""
    _fields_ = [("std_pos", C.c_float), ("std_vel", C.c_float), ("std_meas", C.c_float)]


class TrackSecond(C.Structure):
    """yfv2_track_second (include/yfv2.h): the score classes and the threshold of the tracker's second association pass."""
    _fields_ = [("high_conf", C.c_float), ("low_conf", C.c_float), ("match_thres_low", C.c_double), ("tracked_only", C.c_int32)]


class TrackAppearance(C.Structure):
    """yfv2_track_appearance (include/yfv2.h): the embedding width, the two thresholds and the momentum of the tracker's appearance form."""
    _fields_ = [("dim", C.c_int32), ("prox_thres", C.c_double), ("app_thres", C.c_double), ("alpha", C.c_float)]


class KmeansInfo(C.Structure):
    """yfv2_kmeans_info (include/yfv2.h): what ended yfv2_anchor_kmeans' loop."""
    _fields_ = [("struct_size", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32), ("empty_cluster", C.c_int32),
                ("bad_input", C.c_int32)]


class ApResult(C.Structure):
    """yfv2_ap_result (include/yfv2.h): per-class precision, recall and average precision of a whole validation set."""
    _fields_ = [("struct_size", C.c_int32), ("classes_present", C.c_int32), ("bad_input", C.c_int32),
                ("n_gt", C.c_int64 * 256), ("n_pred", C.c_int64 * 256), ("p", C.c_double * 256), ("r", C.c_double * 256), ("ap", C.c_double * 256),
                ("mean_p", C.c_double), ("mean_r", C.c_double), ("mean_ap", C.c_double), ("mean_f1", C.c_double)]


class Yfv2Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libyfv2 error %d: %s" % (code, msg))
        self.code = code


_PROTOTYPES = {
    # name: (restype, argtypes)
    "yfv2_abi_version": (C.c_int, []),
    "yfv2_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Config)]),
    "yfv2_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Config), C.POINTER(Plan)]),
    "yfv2_destroy": (None, [C.c_void_p]),
    "yfv2_last_error": (C.c_char_p, [C.c_void_p]),
    "yfv2_load_weights": (C.c_int, [C.c_void_p, C.POINTER(TensorDesc), C.c_int32]),
    "yfv2_set_anchors": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "yfv2_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]),
    "yfv2_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]),
    "yfv2_decode": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_double, C.POINTER(C.c_int32), C.c_int32,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]),
    "yfv2_detect_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "yfv2_batch_statistics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                        C.c_void_p, C.c_void_p]),
    "yfv2_batch_statistics_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                              C.c_void_p, C.c_void_p]),
    "yfv2_batch_statistics_overflow": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "yfv2_batch_statistics_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_float),
                                              C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_batch_statistics_multi_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_float),
                                                    C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_nonfinite": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "yfv2_nonfinite_peek": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "yfv2_clock_probe_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    "yfv2_clock_probe_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "yfv2_loss": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "yfv2_train_bind": (C.c_int, [C.c_void_p, C.POINTER(TensorDesc), C.c_int32, C.POINTER(TensorDesc), C.c_int32]),
    "yfv2_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]),
    "yfv2_train_backward": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "yfv2_sgd_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "yfv2_sgd_step_multi": (C.c_int, [C.c_void_p, C.POINTER(SgdItem), C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "yfv2_resize_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_resize_frames_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_detect_frames_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "yfv2_tile_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Tile), C.c_int32]),
    "yfv2_merge_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Tile), C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_detect_tiled_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.POINTER(Tile), C.c_int32, C.c_float, C.c_double, C.c_double,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_resize_frames_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.c_void_p, C.c_void_p]),
    "yfv2_detect_frames_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "yfv2_detect_tiled_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.POINTER(Tile), C.c_int32, C.c_float, C.c_double, C.c_double,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_train_batch_frames_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "yfv2_train_batch_frames_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "yfv2_crop_rect": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_int32)]),
    "yfv2_crop_detections_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CropRule),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "yfv2_crop_detections_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CropRule),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "yfv2_crop_letterbox": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "yfv2_crop_tensor_value": (C.c_int, [C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint16)]),
    "yfv2_crop_tensors_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CropRule),
                                       C.POINTER(CropTensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "yfv2_crop_tensors_yuv": (C.c_int, [C.c_void_p, C.POINTER(FrameYuv), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CropRule),
                                        C.POINTER(CropTensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "yfv2_track_state_words": (C.c_int64, [C.c_int32]),
    "yfv2_track_iou": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "yfv2_track_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                                    C.POINTER(TrackRule), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_track_motion_state_words": (C.c_int64, [C.c_int32]),
    "yfv2_track_filter_step": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(TrackMotion), C.POINTER(C.c_float)]),
    "yfv2_track_birth": (C.c_int, [C.POINTER(C.c_float), C.POINTER(TrackMotion), C.POINTER(C.c_float)]),
    "yfv2_track_update_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                                           C.POINTER(TrackRule), C.POINTER(TrackMotion), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "yfv2_track_update_two_pass": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                                             C.POINTER(TrackRule), C.POINTER(TrackMotion), C.POINTER(TrackSecond), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_track_feature_words": (C.c_int64, [C.c_int32, C.c_int32]),
    "yfv2_track_cosine": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "yfv2_track_feature_step": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_float, C.POINTER(C.c_float),
                                          C.POINTER(C.c_int32)]),
    "yfv2_track_update_appearance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                                               C.POINTER(TrackRule), C.POINTER(TrackMotion), C.POINTER(TrackSecond), C.POINTER(TrackAppearance),
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_export_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yfv2_deploy_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p]),
    "yfv2_deploy_dropped": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "yfv2_detect_deploy_frames_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p]),
    "yfv2_anchor_kmeans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.POINTER(KmeansInfo), C.c_void_p]),
    "yfv2_debug_kmeans_group": (C.c_int, [C.c_void_p, C.c_int32]),
    "yfv2_ap_per_class": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(ApResult), C.c_void_p]),
    "yfv2_ap_per_class_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                          C.POINTER(ApResult), C.c_void_p]),
    "yfv2_debug_plan_dryrun": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "yfv2_debug_plan_dryrun_ex": (C.c_int, [C.c_void_p, C.POINTER(Plan), C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "yfv2_debug_plan_image": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
    "yfv2_debug_plan_image_ex": (C.c_int64, [C.c_void_p, C.POINTER(Plan), C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
    "yfv2_debug_plan_c2_label": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "yfv2_debug_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "yfv2_debug_rows16": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "yfv2_debug_rows_any": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "yfv2_num_rows": (C.c_int32, [C.c_void_p]),
    "yfv2_num_stages": (C.c_int32, [C.c_void_p]),
    "yfv2_stage_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "yfv2_stage_kernel": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32]),
    "yfv2_profile_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_int32,
                                       C.POINTER(C.c_float), C.c_void_p]),
    "yfv2_debug_repeat_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p]),
    "yfv2_debug_post": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "yfv2_debug_activation": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "yfv2_debug_train_relu_output": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "yfv2_debug_train_tensor": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle of libyfv2.so."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: the HIP extension has not been built (run __graft_entry__.build()); "
                          "yolo_fastestv2_amd has no CPU or PyTorch fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    # the ABI number first: a stale build must fail with THIS message, not with an AttributeError on a newer symbol
    if not hasattr(L, "yfv2_abi_version"):
        raise ImportError("%s does not export yfv2_abi_version: not a libyfv2 build" % LIB_PATH)
    L.yfv2_abi_version.restype, L.yfv2_abi_version.argtypes = C.c_int, []
    if L.yfv2_abi_version() != ABI_VERSION:
        raise ImportError("libyfv2.so ABI %d != binding ABI %d: rebuild (__graft_entry__.build())" % (L.yfv2_abi_version(), ABI_VERSION))
    for name, (res, args) in _PROTOTYPES.items():
        if name.startswith("yfv2_debug_") and os.environ.get("YFV2_LIB") and not hasattr(L, name):
            continue  # an older A/B build may lack a host-only test hook; product entry points are never optional
        fn = getattr(L, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error(handle=None):
    msg = lib().yfv2_last_error(handle)
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, handle=None):
    if rc != OK:
        raise Yfv2Error(rc, last_error(handle))
