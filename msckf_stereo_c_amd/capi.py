"""ctypes binding of the C-ABI (include/mskf_hip.h).  Thin: every call goes straight to the HIP
library; there is no Python/CPU fallback and a missing library or device raises."""
import ctypes as C
import os

import numpy as np

from .ctypes_types import (CORNER, DESCRIPTOR_BYTES, EQUALIZE_MODES, EkfDirectArgs, FeDescribeArgs, FeMatchArgs, FeVerifyArgs, IMU_STEP, MATCH, INPUT_FORMAT_BPP, INPUT_FORMATS, ODOM_COV, POINT2F, Calib, EkfCfg, FeCfg, FeEqualize,
                           CAMERA_MODELS, FB_CHECK_MODES, FeCameraModel, FeFbCheck, FeInputFormat, FeMask, FePatchCheck, ImuStep, PATCH_CHECK_MODES, camera_model_cfg, raw_raster)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class MskfError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code        # the mskf_status, when the error came from the library


class TrackArgs(C.Structure):
    _fields_ = [("n", C.c_int32), ("do_temporal", C.c_int32), ("in_pts", C.c_void_p), ("Hpred", C.c_double * 9),
                ("out0", C.c_void_p), ("out1", C.c_void_p), ("und0", C.c_void_p), ("und1", C.c_void_p),
                ("status", C.c_void_p)]


class EkfFeature(C.Structure):
    _fields_ = [("obs_start", C.c_int32), ("n_obs", C.c_int32), ("needs_init", C.c_int32), ("init_start", C.c_int32),
                ("n_init", C.c_int32), ("_pad", C.c_int32), ("position", C.c_double * 3)]


EKF_FEATURE = np.dtype([("obs_start", "<i4"), ("n_obs", "<i4"), ("needs_init", "<i4"), ("init_start", "<i4"),
                        ("n_init", "<i4"), ("_pad", "<i4"), ("position", "<f8", 3)])
CLONE_STATE = np.dtype([("q", "<f8", 4), ("p", "<f8", 3), ("q_null", "<f8", 4), ("p_null", "<f8", 3)])


class EkfUpdateArgs(C.Structure):
    _fields_ = [("n_clones", C.c_int32), ("n_feat", C.c_int32), ("n_obs", C.c_int32), ("dof_offset", C.c_int32),
                ("apply_row_cap", C.c_int32), ("_pad", C.c_int32), ("gravity", C.c_double * 3),
                ("clones", C.c_void_p), ("features", C.c_void_p), ("obs_clone", C.c_void_p), ("obs_z", C.c_void_p),
                ("delta_x", C.c_void_p), ("feat_status", C.c_void_p), ("gamma", C.c_void_p), ("rows_out", C.c_void_p),
                ("diag_out", C.c_void_p), ("pos_var_out", C.c_void_p)]


class FeFrameArgs(C.Structure):   # mskf_fe_frame_args (include/mskf_hip.h)
    _fields_ = [("Hpred", C.c_double * 9), ("capacity", C.c_int32), ("n", C.c_int32),
                ("id", C.c_void_p), ("lifetime", C.c_void_p), ("cam0", C.c_void_p), ("cam1", C.c_void_p), ("und0", C.c_void_p), ("und1", C.c_void_p),
                ("before_tracking", C.c_int32), ("after_tracking", C.c_int32), ("after_matching", C.c_int32), ("after_ransac", C.c_int32),
                ("n_candidates", C.c_int32), ("n_new", C.c_int32), ("next_feature_id", C.c_uint64),
                ("R_p_c", (C.c_double * 9) * 2), ("ransac_draws", C.c_uint64)]


EXPORTS = [
    "mskf_last_error", "mskf_abi_version", "mskf_ctx_create", "mskf_ctx_create_prio", "mskf_ctx_create_shared", "mskf_ctx_destroy", "mskf_ctx_sync", "mskf_ctx_hip_stream",
    "mskf_stream_create", "mskf_stream_destroy", "mskf_fe_push_stereo", "mskf_fe_push_stereo_device",
    "mskf_fe_push_stereo_batch", "mskf_fe_set_detect_floor", "mskf_fe_get_cell_maxima", "mskf_fe_get_cell_candidates", "mskf_fe_track", "mskf_fe_track_batch", "mskf_fe_swap",
    "mskf_fe_get_level", "mskf_ekf_reset", "mskf_ekf_propagate", "mskf_ekf_augment", "mskf_ekf_update",
    "mskf_ekf_update_batch", "mskf_ekf_remove_clone", "mskf_ekf_remove_clones_batch", "mskf_ekf_predict_batch", "mskf_ekf_propagate_imu",
    "mskf_ekf_get_pos_var", "mskf_ekf_get_pos_var_batch", "mskf_ctx_set_timing", "mskf_ctx_get_timing", "mskf_stream_ctx",
    "mskf_ekf_get_dim", "mskf_ekf_get_cov", "mskf_ekf_set_cov", "mskf_ekf_debug_read", "mskf_ctx_get_host_time", "mskf_fe_track_batch_begin", "mskf_fe_track_batch_end",
    "mskf_ekf_update_batch_begin", "mskf_ekf_update_batch_end", "mskf_ekf_get_pos_var_batch_begin", "mskf_ekf_get_pos_var_batch_end", "mskf_ctx_timing_gate",
    "mskf_fe_grid_capacity", "mskf_fe_set_grid", "mskf_fe_frame_batch_begin", "mskf_fe_frame_batch_end", "mskf_ctx_set_wait_mode",
    "mskf_stream_rebind", "mskf_ctx_record_point", "mskf_ctx_wait_point", "mskf_point_destroy", "mskf_ekf_set_compression_mode",
    "mskf_ekf_get_odom_cov", "mskf_ekf_get_odom_cov_batch", "mskf_ekf_get_odom_cov_batch_begin", "mskf_ekf_get_odom_cov_batch_end",
    "mskf_fe_set_equalize", "mskf_fe_get_equalize", "mskf_fe_set_input_format", "mskf_fe_get_input_format",
    "mskf_ekf_update_direct", "mskf_ekf_update_direct_batch", "mskf_ekf_update_direct_batch_begin", "mskf_ekf_update_direct_batch_end",
    "mskf_fe_set_mask", "mskf_fe_get_mask", "mskf_fe_set_patch_check", "mskf_fe_get_patch_check",
    "mskf_fe_set_fb_check", "mskf_fe_get_fb_check", "mskf_fe_set_lk_levels", "mskf_fe_get_lk_levels", "mskf_fe_set_camera_model", "mskf_fe_get_camera_model",
    "mskf_fe_describe", "mskf_fe_describe_batch", "mskf_fe_describe_batch_begin", "mskf_fe_describe_batch_end", "mskf_fe_descriptor_pattern",
    "mskf_fe_match", "mskf_fe_match_batch", "mskf_fe_match_batch_begin", "mskf_fe_match_batch_end",
    "mskf_fe_verify", "mskf_fe_verify_batch", "mskf_fe_verify_batch_begin", "mskf_fe_verify_batch_end",
]


def lib_path():
    return os.path.join(_HERE, "_build", "libmskf_hip.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise MskfError("libmskf_hip.so is not built (run python -m msckf_stereo_c_amd.build); there is no CPU fallback")
        L = C.CDLL(p)
        L.mskf_last_error.restype = C.c_char_p
        L.mskf_ctx_hip_stream.restype = C.c_void_p
        L.mskf_ctx_hip_stream.argtypes = [C.c_void_p]
        L.mskf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.mskf_ctx_destroy.argtypes = [C.c_void_p]
        L.mskf_ctx_sync.argtypes = [C.c_void_p]
        L.mskf_stream_create.argtypes = [C.c_void_p, C.POINTER(Calib), C.POINTER(FeCfg), C.POINTER(EkfCfg), C.POINTER(C.c_void_p)]
        L.mskf_stream_destroy.argtypes = [C.c_void_p]
        L.mskf_fe_push_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
        L.mskf_fe_push_stereo_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        L.mskf_fe_grid_capacity.argtypes = [C.c_void_p]
        L.mskf_fe_set_grid.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p, C.c_uint64]
        L.mskf_fe_frame_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                                C.POINTER(FeFrameArgs)]
        L.mskf_fe_frame_batch_end.argtypes = [C.c_void_p]
        L.mskf_fe_get_cell_maxima.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.mskf_fe_track.argtypes = [C.c_void_p, C.POINTER(TrackArgs)]
        L.mskf_fe_swap.argtypes = [C.c_void_p]
        L.mskf_fe_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mskf_ekf_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.mskf_ekf_propagate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mskf_ekf_augment.argtypes = [C.c_void_p, C.c_void_p]
        L.mskf_ekf_update.argtypes = [C.c_void_p, C.POINTER(EkfUpdateArgs)]
        L.mskf_ekf_remove_clone.argtypes = [C.c_void_p, C.c_int]
        L.mskf_ekf_get_dim.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.mskf_ekf_get_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mskf_ekf_set_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _LIB = L
    return _LIB


def _chk(rc):
    if rc != 0:
        raise MskfError("mskf status %d: %s" % (rc, lib().mskf_last_error().decode()), rc)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _handles(streams):
    """Stream handles as a C array; None stands for a null handle."""
    return (C.c_void_p * len(streams))(*[None if s is None else s.h for s in streams])


def _images(imgs, streams=None):
    """(C array of addresses, what keeps them alive): an entry is a host image in its stream's input format (h x w uint8 by
    default; Stream.set_input_format), a device address, or None."""
    fmts = [0 if streams is None or s is None else s.input_format for s in (imgs if streams is None else streams)]
    keep = [raw_raster(x, f) if isinstance(x, np.ndarray) else x for x, f in zip(imgs, fmts)]
    return (C.c_void_p * len(keep))(*[x.ctypes.data if isinstance(x, np.ndarray) else x for x in keep]), keep


def _pts(a):
    """Points as a contiguous POINT2F array: given as one, or as n x 2 floats."""
    a = np.asarray(a)
    return np.ascontiguousarray(a) if a.dtype == POINT2F else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 2).view(POINT2F).reshape(-1)


def descriptor_pattern():
    """mskf_fe_descriptor_pattern: the 256 tests of the descriptor, (256, 4) int8 of ax, ay, bx, by.  No device call."""
    out = np.zeros((256, 4), np.int8)
    L = lib()
    L.mskf_fe_descriptor_pattern.argtypes = [C.c_void_p]
    L.mskf_fe_descriptor_pattern.restype = None
    L.mskf_fe_descriptor_pattern(_p(out))
    return out


def _describe_args(role, pts):
    """(mskf_fe_describe_args, buffers it points into, (desc, valid) the call fills) for one stream."""
    pts = _pts(np.zeros((0, 2), np.float32) if pts is None else pts)
    n = len(pts)
    desc, valid = np.zeros((n, DESCRIPTOR_BYTES), np.uint8), np.zeros(n, np.uint8)
    a = FeDescribeArgs(int(role), n, pts.ctypes.data if n else None, desc.ctypes.data if n else None, valid.ctypes.data if n else None)
    return a, pts, (desc, valid)


def _descriptor_set(desc, valid):
    """(uint8[n, 32] contiguous, uint8[n] contiguous or None) of a descriptor set; arrays that already are so are passed as they are,
    so that jobs naming the same array share one copy on the device."""
    d = desc if isinstance(desc, np.ndarray) and desc.dtype == np.uint8 and desc.flags.c_contiguous else np.ascontiguousarray(desc, dtype=np.uint8)
    d = d.reshape(-1, DESCRIPTOR_BYTES)
    if valid is None:
        return d, None
    v = valid if isinstance(valid, np.ndarray) and valid.dtype == np.uint8 and valid.flags.c_contiguous else np.ascontiguousarray(valid, dtype=np.uint8)
    v = v.reshape(-1)
    if len(v) != len(d):
        raise ValueError("a validity array has one byte per descriptor")
    return d, v


def _match_args(job):
    """(mskf_fe_match_args, buffers it points into, matches the call fills) for one job: a dict with query, train and optionally
    query_valid, train_valid, max_distance (256), ratio (0 = off), cross_check (False)."""
    q, qv = _descriptor_set(job["query"], job.get("query_valid"))
    t, tv = _descriptor_set(job["train"], job.get("train_valid"))
    m = np.zeros(len(q), MATCH)
    a = FeMatchArgs(len(q), len(t), q.ctypes.data if len(q) else None, None if qv is None or not len(q) else qv.ctypes.data,
                    t.ctypes.data if len(t) else None, None if tv is None or not len(t) else tv.ctypes.data,
                    int(job.get("max_distance", 256)), float(job.get("ratio", 0.0)), int(bool(job.get("cross_check", False))),
                    m.ctypes.data if len(q) else None, -1)
    return a, (q, qv, t, tv), m


def _verify_args(job):
    """(mskf_fe_verify_args, buffers it points into, inlier bytes the call fills) for one job: a dict with query_obs, train_obs
    (float64[n, 4]: x0, y0, x1, y1 normalised), T_cam1_cam0 (16 doubles, row-major) and optionally usable (uint8[n]), n_hypotheses
    (256), seed (0), max_error (normalised units; required), min_depth (0.1), max_depth (40.0)."""
    q = np.ascontiguousarray(job["query_obs"], dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(job["train_obs"], dtype=np.float64).reshape(-1, 4)
    if len(q) != len(t):
        raise ValueError("a pair has one observation on each side")
    u = job.get("usable")
    if u is not None:
        u = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1)
        if len(u) != len(q):
            raise ValueError("a usable array has one byte per pair")
    inl = np.zeros(len(q), np.uint8)
    a = FeVerifyArgs()
    a.n, a.n_hypotheses = len(q), int(job.get("n_hypotheses", 256))
    a.query_obs, a.train_obs = (q.ctypes.data, t.ctypes.data) if len(q) else (None, None)
    a.usable = None if u is None or not len(q) else u.ctypes.data
    a.T_cam1_cam0[:] = [float(v) for v in np.asarray(job["T_cam1_cam0"], dtype=np.float64).reshape(-1)]
    a.seed = int(job.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
    a.max_error, a.min_depth, a.max_depth = float(job["max_error"]), float(job.get("min_depth", 0.1)), float(job.get("max_depth", 40.0))
    a.inlier = inl.ctypes.data if len(q) else None
    a.n_usable = a.n_inliers = a.status = -9
    a.best = -9
    return a, (q, t, u), inl


def _verify_result(a, inl):
    """What a verify call returns for one job."""
    return dict(n_usable=int(a.n_usable), n_inliers=int(a.n_inliers), best=int(a.best), status=int(a.status), inlier=inl,
                R=np.array(a.R[:], np.float64).reshape(3, 3), t=np.array(a.t[:], np.float64), info=np.array(a.info[:], np.float64).reshape(6, 6), rms=float(a.rms))


def _imu_steps(steps):
    """mskf_imu_step records as a contiguous IMU_STEP array (None / empty: no steps)."""
    if steps is None:
        return np.zeros(0, IMU_STEP)
    a = np.ascontiguousarray(steps)
    assert a.dtype == IMU_STEP and a.ndim == 1, a.dtype
    return a


class Context:
    def __init__(self, device=0, shared_with=None):
        """shared_with: a parent Context whose HIP stream this one enqueues on (mskf_ctx_create_shared; close it first)."""
        self.L = lib()
        self.h = C.c_void_p()
        if shared_with is None:
            _chk(self.L.mskf_ctx_create(device, C.byref(self.h)))
        else:
            self.L.mskf_ctx_create_shared.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            _chk(self.L.mskf_ctx_create_shared(shared_with.h, C.byref(self.h)))
        self.streams = []
        self._trk_pending = None
        self._frame_pending = None
        self._direct_pending = None
        self._dsc_pending = None
        self._mch_pending = None
        self._vfy_pending = None

    def close(self):
        if self.h:
            for s in list(self.streams):
                s.close()
            self.L.mskf_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        _chk(self.L.mskf_ctx_sync(self.h))

    def ekf_update_batch(self, streams, problems):
        """One mskf_ekf_update_batch over several streams of this context; problems[i] = kwargs of Stream.ekf_update."""
        n = len(streams)
        built = [Stream._update_args(**pr) for pr in problems]
        args = (EkfUpdateArgs * n)(*[b[0] for b in built])
        hs = (C.c_void_p * n)(*[s.h for s in streams])
        self.L.mskf_ekf_update_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(EkfUpdateArgs)]
        _chk(self.L.mskf_ekf_update_batch(self.h, n, hs, args))
        return [b[2]() for b in built]

    def _track_batch_args(self, streams, problems):
        n = len(streams)
        built = [Stream._track_args(**pr) for pr in problems]
        args = (TrackArgs * n)(*[b[0] for b in built])
        hs = (C.c_void_p * n)(*[s.h for s in streams])
        return n, built, args, hs

    def track_batch(self, streams, problems):
        """One mskf_fe_track_batch over several streams of this context; problems[i] = kwargs of Stream.track."""
        n, built, args, hs = self._track_batch_args(streams, problems)
        self.L.mskf_fe_track_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(TrackArgs)]
        _chk(self.L.mskf_fe_track_batch(self.h, n, hs, args))
        return [b[2] for b in built]

    def track_batch_begin(self, streams, problems):
        """mskf_fe_track_batch_begin: enqueue the batch; the returned result dicts are filled by track_batch_end."""
        n, built, args, hs = self._track_batch_args(streams, problems)
        self.L.mskf_fe_track_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(TrackArgs)]
        _chk(self.L.mskf_fe_track_batch_begin(self.h, n, hs, args))
        self._trk_pending = (built, args, hs)          # must stay alive until _end
        return [b[2] for b in built]

    def track_batch_end(self):
        self.L.mskf_fe_track_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_fe_track_batch_end(self.h))
        self._trk_pending = None

    def describe_batch(self, streams, roles, pts_list):
        """One mskf_fe_describe_batch: 256-bit descriptors of pts_list[i] (n x 2 level-0 pixels, None = none) on the image roles[i]
        (0 prev cam0, 1 curr cam0, 2 curr cam1) of streams[i].  Returns [(desc uint8[n, 32], valid uint8[n])]."""
        out = self.describe_batch_begin(streams, roles, pts_list)
        self.describe_batch_end()
        return out

    def describe_batch_begin(self, streams, roles, pts_list):
        """mskf_fe_describe_batch_begin: enqueue the batch; the returned arrays are filled by describe_batch_end."""
        n = len(streams)
        built = [_describe_args(r, p) for r, p in zip(roles, pts_list)]
        args = (FeDescribeArgs * n)(*[b[0] for b in built])
        hs = _handles(streams)
        self.L.mskf_fe_describe_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(FeDescribeArgs)]
        _chk(self.L.mskf_fe_describe_batch_begin(self.h, n, hs, args))
        self._dsc_pending = (built, args, hs)          # must stay alive until _end
        return [b[2] for b in built]

    def describe_batch_end(self):
        self.L.mskf_fe_describe_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_fe_describe_batch_end(self.h))
        self._dsc_pending = None

    def match_batch(self, jobs):
        """One mskf_fe_match_batch: brute-force Hamming matching of 256-bit descriptors, a job per dict of jobs (query, train uint8[n, 32];
        optional query_valid, train_valid uint8[n], max_distance = 256, ratio = 0.0 (off), cross_check = False).  Jobs that name the same
        array share one copy on the device.  Returns [(matches MATCH[nq], n_matches)]: idx = the accepted train index or -1, nearest /
        dist / second the raw nearest neighbour (lowest index among equal distances), its distance and the next smallest distance."""
        self.match_batch_begin(jobs)
        return self.match_batch_end()

    def match_batch_begin(self, jobs):
        """mskf_fe_match_batch_begin: enqueue the batch; match_batch_end returns the results."""
        built = [_match_args(j) for j in jobs]
        n = len(built)
        args = (FeMatchArgs * max(n, 1))(*[b[0] for b in built])
        self.L.mskf_fe_match_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeMatchArgs)]
        _chk(self.L.mskf_fe_match_batch_begin(self.h, n, args))
        self._mch_pending = (built, args)             # must stay alive until _end
        return [b[2] for b in built]

    def match_batch_end(self):
        """mskf_fe_match_batch_end: [(matches, n_matches)] of the batch begun, None when there was none."""
        self.L.mskf_fe_match_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_fe_match_batch_end(self.h))
        pend, self._mch_pending = self._mch_pending, None
        if pend is None:
            return None
        built, args = pend
        return [(b[2], int(args[i].n_matches)) for i, b in enumerate(built)]

    def match(self, query, train, query_valid=None, train_valid=None, max_distance=256, ratio=0.0, cross_check=False):
        """mskf_fe_match: one job; returns (matches MATCH[nq], n_matches); synchronises."""
        a, _keep, m = _match_args(dict(query=query, train=train, query_valid=query_valid, train_valid=train_valid, max_distance=max_distance,
                                       ratio=ratio, cross_check=cross_check))
        self.L.mskf_fe_match.argtypes = [C.c_void_p, C.POINTER(FeMatchArgs)]
        _chk(self.L.mskf_fe_match(self.h, C.byref(a)))
        return m, int(a.n_matches)

    def verify_batch(self, jobs):
        """One mskf_fe_verify_batch: the stereo RANSAC pose check of matched pairs ("Geometric verification"), a
        job per dict of jobs (see _verify_args).  Returns a dict per job: n_usable, n_inliers, best (the winning hypothesis or -1),
        status (0 ok, 1 no hypothesis, 2 refinement failed), inlier uint8[n] at the original indices, R (3, 3) and t with
        p_keyframe = R p_query + t in cam0 coordinates, info (6, 6; J^T J in the order [theta, t]) and rms."""
        self.verify_batch_begin(jobs)
        return self.verify_batch_end()

    def verify_batch_begin(self, jobs):
        """mskf_fe_verify_batch_begin: stage and enqueue the batch; verify_batch_end returns the results."""
        built = [_verify_args(j) for j in jobs]
        n = len(built)
        args = (FeVerifyArgs * max(n, 1))(*[b[0] for b in built])
        self.L.mskf_fe_verify_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeVerifyArgs)]
        _chk(self.L.mskf_fe_verify_batch_begin(self.h, n, args))
        self._vfy_pending = (built, args)             # must stay alive until _end

    def verify_batch_end(self):
        """mskf_fe_verify_batch_end: the results of the batch begun, None when there was none."""
        self.L.mskf_fe_verify_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_fe_verify_batch_end(self.h))
        pend, self._vfy_pending = self._vfy_pending, None
        if pend is None:
            return None
        built, args = pend
        return [_verify_result(args[i], b[2]) for i, b in enumerate(built)]

    def verify(self, query_obs, train_obs, T_cam1_cam0, max_error, usable=None, n_hypotheses=256, seed=0, min_depth=0.1, max_depth=40.0):
        """mskf_fe_verify: one job; returns its result dict (verify_batch); synchronises."""
        a, _keep, inl = _verify_args(dict(query_obs=query_obs, train_obs=train_obs, T_cam1_cam0=T_cam1_cam0, max_error=max_error, usable=usable,
                                          n_hypotheses=n_hypotheses, seed=seed, min_depth=min_depth, max_depth=max_depth))
        self.L.mskf_fe_verify.argtypes = [C.c_void_p, C.POINTER(FeVerifyArgs)]
        _chk(self.L.mskf_fe_verify(self.h, C.byref(a)))
        return _verify_result(a, inl)

    def push_stereo_batch(self, streams, cam0s, cam1s, on_device=0):
        """One mskf_fe_push_stereo_batch: host images (on_device = 0) or device addresses (1: copied, 2: borrowed)."""
        a, _keep_a = _images(cam0s, streams)
        b, _keep_b = _images(cam1s, streams)
        _chk(self.L.mskf_fe_push_stereo_batch(self.h, len(streams), _handles(streams), a, b, on_device))

    def frame_batch_begin(self, streams, images, args, on_device=0):
        """mskf_fe_frame_batch_begin: a whole front-end frame of every stream on the device.  images[i] = (cam0, cam1) as for
        push_stereo_batch; args[i] = dict(Hpred=3 x 3 or None for the identity, R_p_c=2 x 3 x 3 or None, capacity=entries of the
        output arrays or None for the stream's grid_capacity()).  frame_batch_end returns the results."""
        n = len(streams)
        a, keep_a = _images([im[0] for im in images], streams)
        b, keep_b = _images([im[1] for im in images], streams)
        fa = (FeFrameArgs * n)()
        outs = []
        for i, (s, kw) in enumerate(zip(streams, args)):
            cap = kw.get("capacity")
            cap = (s.grid_capacity() if s is not None else 0) if cap is None else cap
            o = dict(id=np.zeros(max(cap, 1), np.uint64), lifetime=np.zeros(max(cap, 1), np.int32),
                     **{k: np.zeros(max(cap, 1), POINT2F) for k in ("cam0", "cam1", "und0", "und1")})
            H = np.eye(3) if kw.get("Hpred") is None else np.ascontiguousarray(kw["Hpred"], dtype=np.float64)
            R = np.stack([np.eye(3)] * 2) if kw.get("R_p_c") is None else np.ascontiguousarray(kw["R_p_c"], dtype=np.float64)
            fa[i].Hpred[:] = list(H.reshape(-1))
            for c in range(2):
                fa[i].R_p_c[c][:] = list(R.reshape(2, 9)[c])
            fa[i].capacity = cap
            for k, v in o.items():
                setattr(fa[i], k, v.ctypes.data)
            outs.append(o)
        hs = _handles(streams)
        _chk(self.L.mskf_fe_frame_batch_begin(self.h, n, hs, a, b, on_device, fa))
        self._frame_pending = (fa, outs, hs, a, b, keep_a, keep_b)          # must stay alive until _end
        return outs

    def frame_batch_end(self):
        """Per stream of the pending frame batch: the published grid (arrays cut to n) and the frame's counters."""
        _chk(self.L.mskf_fe_frame_batch_end(self.h))
        pending, self._frame_pending = self._frame_pending, None
        if pending is None:
            return []
        res = []
        for a, o in zip(pending[0], pending[1]):
            r = {k: v[:a.n].copy() if v.dtype != POINT2F else v[:a.n].view(np.float32).reshape(-1, 2).copy() for k, v in o.items()}
            r.update({k: int(getattr(a, k)) for k in ("n", "before_tracking", "after_tracking", "after_matching", "after_ransac", "n_candidates", "n_new",
                                                      "next_feature_id", "ransac_draws")})
            res.append(r)
        return res

    def ekf_predict_batch(self, streams, steps, J):
        """One mskf_ekf_predict_batch: streams[i] propagates over steps[i] (IMU_STEP records, None = none), then augments
        with J[i] (6 x 21, None = no augmentation)."""
        n = len(streams)
        st = [_imu_steps(x) for x in steps]
        Js = [None if j is None else np.ascontiguousarray(j, dtype=np.float64).reshape(6, 21) for j in J]
        hs = (C.c_void_p * n)(*[s.h for s in streams])
        ns = (C.c_int32 * n)(*[len(x) for x in st])
        sp = (C.c_void_p * n)(*[x.ctypes.data if len(x) else None for x in st])
        jp = (C.c_void_p * n)(*[None if j is None else j.ctypes.data for j in Js])
        self.L.mskf_ekf_predict_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        _chk(self.L.mskf_ekf_predict_batch(self.h, n, hs, ns, sp, jp))

    def ekf_remove_clones_batch(self, streams, pairs):
        """One mskf_ekf_remove_clones_batch: pairs[i] = (a, b) clone indices of streams[i] in the current order, -1 = none."""
        n = len(streams)
        idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(n, 2))
        hs = (C.c_void_p * n)(*[s.h for s in streams])
        self.L.mskf_ekf_remove_clones_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
        _chk(self.L.mskf_ekf_remove_clones_batch(self.h, n, hs, _p(idx)))

    def ekf_pos_var_batch(self, streams):
        """P(12,12), P(13,13), P(14,14) of every stream, (n, 3)."""
        out = self.ekf_pos_var_batch_begin(streams)
        self.ekf_pos_var_batch_end()
        return out

    def ekf_pos_var_batch_begin(self, streams):
        """Enqueue the read-out; the returned (n, 3) array is filled by ekf_pos_var_batch_end."""
        n = len(streams)
        out = np.full((n, 3), np.nan)
        hs = (C.c_void_p * n)(*[s.h for s in streams])
        self.L.mskf_ekf_get_pos_var_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
        _chk(self.L.mskf_ekf_get_pos_var_batch_begin(self.h, n, hs, _p(out)))
        self._pv_pending = (out, hs)          # both must stay alive until _end
        return out

    def ekf_pos_var_batch_end(self):
        self.L.mskf_ekf_get_pos_var_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_ekf_get_pos_var_batch_end(self.h))
        self._pv_pending = None

    def ekf_odom_cov_batch(self, streams):
        """The published pose / velocity covariance of every stream (mskf_odom_cov), an ODOM_COV array of n records."""
        out = self.ekf_odom_cov_batch_begin(streams)
        self.ekf_odom_cov_batch_end()
        return out

    def ekf_odom_cov_batch_begin(self, streams, out=None):
        """Enqueue the read-out; the returned ODOM_COV array (or `out`, if given) is filled by ekf_odom_cov_batch_end."""
        n = len(streams)
        if out is None:
            out = np.zeros(n, ODOM_COV)
            out.view(np.float64)[:] = np.nan
        self.L.mskf_ekf_get_odom_cov_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
        hs = _handles(streams)
        _chk(self.L.mskf_ekf_get_odom_cov_batch_begin(self.h, n, hs, _p(out)))
        self._oc_pending = (out, hs)          # both must stay alive until _end
        return out

    def ekf_odom_cov_batch_end(self):
        self.L.mskf_ekf_get_odom_cov_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_ekf_get_odom_cov_batch_end(self.h))
        self._oc_pending = None

    def ekf_update_direct_batch(self, streams, problems):
        """One mskf_ekf_update_direct_batch over several streams of this context; problems[i] = kwargs of Stream.ekf_update_direct,
        or None for a stream that takes no part (m = 0).  Returns the result dicts."""
        out = self.ekf_update_direct_batch_begin(streams, problems)
        self.ekf_update_direct_batch_end()
        return out

    def ekf_update_direct_batch_begin(self, streams, problems):
        """mskf_ekf_update_direct_batch_begin: enqueue the batch; the returned result dicts are filled by ekf_update_direct_batch_end."""
        n = len(streams)
        built = [Stream._direct_args(s, **(pr or {})) for s, pr in zip(streams, problems)]
        args = (EkfDirectArgs * n)(*[b[0] for b in built])
        hs = _handles(streams)
        self.L.mskf_ekf_update_direct_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(EkfDirectArgs)]
        _chk(self.L.mskf_ekf_update_direct_batch_begin(self.h, n, hs, args))
        self._direct_pending = (built, args, hs)          # must stay alive until _end
        return [b[2] for b in built]

    def ekf_update_direct_batch_end(self):
        self.L.mskf_ekf_update_direct_batch_end.argtypes = [C.c_void_p]
        _chk(self.L.mskf_ekf_update_direct_batch_end(self.h))
        pending, self._direct_pending = self._direct_pending, None
        if pending is not None:
            for a, b in zip(pending[1], pending[0]):
                b[2]["gamma"], b[2]["status"] = float(a.gamma), int(a.status)

    def hip_stream(self):
        return self.L.mskf_ctx_hip_stream(self.h)

    def launch_copy(self, dst, src, nbytes):
        """k_mskf_copy of up to 6 segments (device or pinned host addresses, 16-byte aligned) in one launch on this context's
        HIP stream (fe_launch_copy: the staging copies of the hot path).  Asynchronous: sync() before reading."""
        n = len(dst)
        assert len(src) == n == len(nbytes)
        self.L.fe_launch_copy.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p]
        self.L.fe_launch_copy.restype = None
        self.L.fe_launch_copy((C.c_void_p * n)(*dst), (C.c_void_p * n)(*src), (C.c_size_t * n)(*nbytes), n, self.hip_stream())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """One VIO stream: device-resident pyramids + covariance behind the C-ABI."""

    def __init__(self, ctx, calib, fe_cfg, ekf_cfg):
        self.ctx, self.L = ctx, ctx.L
        self.calib, self.fe_cfg, self.ekf_cfg = calib, fe_cfg, ekf_cfg
        self.h = C.c_void_p()
        self.input_format = 0          # MSKF_PIX_GRAY8 (set_input_format keeps it)
        _chk(self.L.mskf_stream_create(ctx.h, C.byref(calib), C.byref(fe_cfg), C.byref(ekf_cfg), C.byref(self.h)))
        ctx.streams.append(self)

    def close(self):
        if self.h:
            self.L.mskf_stream_destroy(self.h)
            self.h = None
            if self in self.ctx.streams:
                self.ctx.streams.remove(self)

    # ---- front-end
    def push_stereo(self, cam0, cam1, t=0.0, pitch=None):
        """cam0 / cam1: h x w images, or (pitch given) h x pitch buffers whose first w = calib.width columns are the image.
        With an input format (set_input_format): images of its dtype and shape ((h, w) uint16, (h, w, 3 | 4) uint8, (h, w) uint8),
        or (pitch given) h x pitch uint8 buffers of raw bytes whose first w * bytes-per-pixel columns are the image."""
        if pitch is not None:
            cam0, cam1 = np.ascontiguousarray(cam0, dtype=np.uint8), np.ascontiguousarray(cam1, dtype=np.uint8)
            assert cam0.ndim == 2 and cam0.shape[1] == pitch and cam1.shape == cam0.shape
            h, w = cam0.shape[0], self.calib.width
        else:
            cam0, cam1 = raw_raster(cam0, self.input_format), raw_raster(cam1, self.input_format)
            assert cam1.shape == cam0.shape
            h, w = cam0.shape[:2]
        _chk(self.L.mskf_fe_push_stereo(self.h, _p(cam0), _p(cam1), w, h, w * INPUT_FORMAT_BPP[self.input_format] if pitch is None else pitch, t))

    def grid_capacity(self):
        """Entries a published grid of this stream can have; 0: the stream keeps its books on the host."""
        return self.L.mskf_fe_grid_capacity(self.h)

    def set_grid(self, id=None, lifetime=None, cam0=None, cam1=None, und0=None, und1=None, next_feature_id=0, tracking_counters=None,
                 ransac_draws=0, n=None):
        """mskf_fe_set_grid: hand the device the grid a host-side frame has published (no arrays: an empty grid)."""
        arrs = [None if id is None else np.ascontiguousarray(id, dtype=np.uint64), None if lifetime is None else np.ascontiguousarray(lifetime, dtype=np.int32)]
        arrs += [None if x is None else _pts(x) for x in (cam0, cam1, und0, und1)]
        if n is None:
            n = 0 if arrs[0] is None else len(arrs[0])
        tc = None if tracking_counters is None else np.ascontiguousarray(tracking_counters, dtype=np.int32)
        _chk(self.L.mskf_fe_set_grid(self.h, n, *[None if x is None else _p(x) for x in arrs], next_feature_id, None if tc is None else _p(tc), ransac_draws))

    def set_detect_floor(self, min_score):
        _chk(self.L.mskf_fe_set_detect_floor(self.h, int(min_score)))

    def set_equalize(self, mode, tiles=(8, 8), clip_limit=40.0):
        """mskf_fe_set_equalize: mode 0 / "off", 1 / "hist" (global), 2 / "clahe"; tiles = (tiles_x, tiles_y).  From the next push on."""
        cfg = FeEqualize(int(EQUALIZE_MODES.get(mode, mode)), int(tiles[0]), int(tiles[1]), 0, float(clip_limit))
        self.L.mskf_fe_set_equalize.argtypes = [C.c_void_p, C.POINTER(FeEqualize)]
        _chk(self.L.mskf_fe_set_equalize(self.h, C.byref(cfg)))

    def get_equalize(self):
        """(mode, (tiles_x, tiles_y), clip_limit) as the stream holds them."""
        cfg = FeEqualize()
        self.L.mskf_fe_get_equalize.argtypes = [C.c_void_p, C.POINTER(FeEqualize)]
        _chk(self.L.mskf_fe_get_equalize(self.h, C.byref(cfg)))
        return cfg.mode, (cfg.tiles_x, cfg.tiles_y), cfg.clip_limit

    def set_input_format(self, fmt, shift=0):
        """mskf_fe_set_input_format: fmt is a name ("gray8", "gray16", "rgb8", "bgr8", "rgba8", "bgra8", "bayer_rggb8", "bayer_grbg8",
        "bayer_gbrg8", "bayer_bggr8") or its number; shift (0 .. 8) goes with gray16: g = min(v >> shift, 255).  From the next push on."""
        if isinstance(fmt, str) and fmt not in INPUT_FORMATS:
            raise MskfError("unknown input format %r" % (fmt,), -1)
        cfg = FeInputFormat(int(INPUT_FORMATS.get(fmt, fmt)), int(shift))
        self.L.mskf_fe_set_input_format.argtypes = [C.c_void_p, C.POINTER(FeInputFormat)]
        _chk(self.L.mskf_fe_set_input_format(self.h, C.byref(cfg)))
        self.input_format = cfg.format

    def get_input_format(self):
        """(format number, shift) as the stream holds them."""
        cfg = FeInputFormat()
        self.L.mskf_fe_get_input_format.argtypes = [C.c_void_p, C.POINTER(FeInputFormat)]
        _chk(self.L.mskf_fe_get_input_format(self.h, C.byref(cfg)))
        return cfg.format, cfg.shift

    def set_mask(self, cam0=None, cam1=None, margin=0):
        """mskf_fe_set_mask: per-camera image masks, (h, w) arrays in which a pixel != 0 is USABLE and 0 is masked out (bool arrays
        too); None = that camera is not masked, both None = off.  margin (0 .. 64) erodes the usable set; a detector score reads
        5 pixels around its pixel, so a mask or its margin should reach that far beyond a hard edge.  The detector takes it from the
        next push on, the point gate from the next track or frame call."""
        planes = [None if m is None else np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8) for m in (cam0, cam1)]
        shapes = {m.shape for m in planes if m is not None}
        if len(shapes) > 1 or any(m.ndim != 2 for m in planes if m is not None):
            raise MskfError("the masks are 2-D planes of one size", -1)
        h, w = shapes.pop() if shapes else (0, 0)
        cfg = FeMask(None if planes[0] is None else planes[0].ctypes.data, None if planes[1] is None else planes[1].ctypes.data, w, h, w, int(margin))
        self.L.mskf_fe_set_mask.argtypes = [C.c_void_p, C.POINTER(FeMask)]
        _chk(self.L.mskf_fe_set_mask(self.h, C.byref(cfg)))

    def get_mask(self, cam):
        """(mask, margin): the eroded mask of camera 0 / 1 as the stream holds it, (h, w) uint8 of 0 / 255, or None without one."""
        w, h, margin = C.c_int(), C.c_int(), C.c_int()
        out = np.zeros((self.calib.height, self.calib.width), np.uint8)
        self.L.mskf_fe_get_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 3
        _chk(self.L.mskf_fe_get_mask(self.h, int(cam), _p(out), out.size, C.byref(w), C.byref(h), C.byref(margin)))
        if w.value == 0:
            return None, margin.value
        assert (h.value, w.value) == out.shape
        return out, margin.value

    def set_patch_check(self, mode="both", half=4, min_zncc_temporal=0.8, min_zncc_stereo=0.8):
        """mskf_fe_set_patch_check: the ZNCC patch check behind every track launch; mode "both" / "temporal" / "stereo" / "off" (or
        the bits 1 | 2), half 2 .. 7 (a patch is (2 half + 1)^2 samples), thresholds in [0, 1].  From the next track or frame call on."""
        if isinstance(mode, str) and mode not in PATCH_CHECK_MODES:
            raise MskfError("unknown patch check mode %r" % (mode,), -1)
        cfg = FePatchCheck(int(PATCH_CHECK_MODES.get(mode, mode)), int(half), float(min_zncc_temporal), float(min_zncc_stereo))
        self.L.mskf_fe_set_patch_check.argtypes = [C.c_void_p, C.POINTER(FePatchCheck)]
        _chk(self.L.mskf_fe_set_patch_check(self.h, C.byref(cfg)))

    def get_patch_check(self):
        """(mode bits, half, min_zncc_temporal, min_zncc_stereo) as the stream holds them."""
        cfg = FePatchCheck()
        self.L.mskf_fe_get_patch_check.argtypes = [C.c_void_p, C.POINTER(FePatchCheck)]
        _chk(self.L.mskf_fe_get_patch_check(self.h, C.byref(cfg)))
        return cfg.mode, cfg.half, cfg.min_zncc_temporal, cfg.min_zncc_stereo

    def set_fb_check(self, mode="both", max_error_temporal=1.0, max_error_stereo=1.0):
        """mskf_fe_set_fb_check: the forward-backward check behind every track launch (the result is tracked back from the known
        origin and must return to it); mode "both" / "temporal" / "stereo" / "off" (or the bits 1 | 2), thresholds in level-0
        pixels, 0 .. 64.  From the next track or frame call on."""
        if isinstance(mode, str) and mode not in FB_CHECK_MODES:
            raise MskfError("unknown forward-backward check mode %r" % (mode,), -1)
        cfg = FeFbCheck(int(FB_CHECK_MODES.get(mode, mode)), float(max_error_temporal), float(max_error_stereo))
        self.L.mskf_fe_set_fb_check.argtypes = [C.c_void_p, C.POINTER(FeFbCheck)]
        _chk(self.L.mskf_fe_set_fb_check(self.h, C.byref(cfg)))

    def get_fb_check(self):
        """(mode bits, max_error_temporal, max_error_stereo) as the stream holds them."""
        cfg = FeFbCheck()
        self.L.mskf_fe_get_fb_check.argtypes = [C.c_void_p, C.POINTER(FeFbCheck)]
        _chk(self.L.mskf_fe_get_fb_check(self.h, C.byref(cfg)))
        return cfg.mode, cfg.max_error_temporal, cfg.max_error_stereo

    def set_lk_levels(self, levels):
        """mskf_fe_set_lk_levels: every pyramidal LK of the stream (temporal track, both stereo matches, the backward tracks of the
        forward-backward check) runs over `levels` = 4 .. 8 pyramid levels; 4 is the default.  Refused for a depth whose top level
        has a side below 15 pixels at the stream's size, and after the stream's first push."""
        self.L.mskf_fe_set_lk_levels.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.mskf_fe_set_lk_levels(self.h, int(levels)))

    def get_lk_levels(self):
        """The number of LK pyramid levels as the stream holds it (a stream never set: 4)."""
        n = C.c_int(0)
        self.L.mskf_fe_get_lk_levels.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _chk(self.L.mskf_fe_get_lk_levels(self.h, C.byref(n)))
        return n.value

    def set_camera_model(self, cam, model, coeffs):
        """mskf_fe_set_camera_model: camera `cam` (0 / 1) takes the model "radtan" | "equidistant" (4 coefficients: back on the base
        path) | "radtan8" (OpenCV's 5 or 8: k1 k2 p1 p2 k3 [k4 k5 k6]) | "fov" (w) | "ds" (xi, alpha); the intrinsics stay the
        calibration's.  From the next track or frame call on."""
        try:
            cfg = camera_model_cfg(cam, model, coeffs)
        except ValueError as e:
            raise MskfError(str(e), -1)
        self.L.mskf_fe_set_camera_model.argtypes = [C.c_void_p, C.POINTER(FeCameraModel)]
        _chk(self.L.mskf_fe_set_camera_model(self.h, C.byref(cfg)))

    def get_camera_model(self, cam):
        """(model name, the eight coefficients as the stream holds them) of camera `cam`."""
        cfg = FeCameraModel()
        self.L.mskf_fe_get_camera_model.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeCameraModel)]
        _chk(self.L.mskf_fe_get_camera_model(self.h, int(cam), C.byref(cfg)))
        names = {v: k for k, v in CAMERA_MODELS.items()}
        return names.get(cfg.model, cfg.model), [float(v) for v in cfg.coeffs]

    def describe(self, role, pts):
        """mskf_fe_describe: the 256-bit descriptors of pts (n x 2, level-0 pixels) on the image `role` (0 prev cam0, 1 curr cam0,
        2 curr cam1) as get_level(role, 0) returns it.  Returns (desc uint8[n, 32], valid uint8[n]); synchronises."""
        a, _keep, out = _describe_args(role, pts)
        self.L.mskf_fe_describe.argtypes = [C.c_void_p, C.POINTER(FeDescribeArgs)]
        _chk(self.L.mskf_fe_describe(self.h, C.byref(a)))
        return out

    def cell_maxima(self):
        n = self.fe_cfg.det_rows * self.fe_cfg.det_cols
        out = np.zeros(n, CORNER)
        got = C.c_int()
        _chk(self.L.mskf_fe_get_cell_maxima(self.h, _p(out), n, C.byref(got)))
        return out[:got.value]

    def cell_candidates(self, min_score):
        """Per-cell maxima whose score exceeds min_score (1/256 units), in cell order."""
        n = self.fe_cfg.det_rows * self.fe_cfg.det_cols
        out = np.zeros(n, CORNER)
        got = C.c_int()
        self.L.mskf_fe_get_cell_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _chk(self.L.mskf_fe_get_cell_candidates(self.h, int(min_score), _p(out), n, C.byref(got)))
        return out[:got.value]

    @staticmethod
    def _track_args(pts, do_temporal, Hpred=None):
        """(mskf_fe_track_args, buffers it points into, result dict the call fills) for one stream."""
        pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        out0, out1, und0, und1 = (np.zeros((n, 2), np.float32) for _ in range(4))
        status = np.zeros(n, np.uint8)
        a = TrackArgs()
        a.n, a.do_temporal = n, int(do_temporal)
        a.in_pts = pts.ctypes.data
        H = np.eye(3) if Hpred is None else np.ascontiguousarray(Hpred, dtype=np.float64)
        a.Hpred[:] = list(H.reshape(-1))
        a.out0, a.out1, a.und0, a.und1, a.status = (x.ctypes.data for x in (out0, out1, und0, und1, status))
        return a, pts, dict(out0=out0, out1=out1, und0=und0, und1=und1, status=status)

    def track(self, pts, do_temporal, Hpred=None):
        a, _keep, result = self._track_args(pts, do_temporal, Hpred)
        _chk(self.L.mskf_fe_track(self.h, C.byref(a)))
        return result

    def swap(self):
        _chk(self.L.mskf_fe_swap(self.h))

    def get_level(self, role, level):
        w, h = C.c_int(), C.c_int()
        buf = np.zeros(self.calib.width * self.calib.height, np.uint8)
        _chk(self.L.mskf_fe_get_level(self.h, role, level, _p(buf), buf.size, C.byref(w), C.byref(h)))
        return buf[:w.value * h.value].reshape(h.value, w.value).copy()

    # ---- EKF
    def ekf_reset(self, P0):
        P0 = np.ascontiguousarray(P0, dtype=np.float64)
        assert P0.shape == (21, 21)
        _chk(self.L.mskf_ekf_reset(self.h, _p(P0)))

    def ekf_set_cov(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        _chk(self.L.mskf_ekf_set_cov(self.h, _p(P), P.shape[0]))

    def ekf_dim(self):
        d = C.c_int()
        _chk(self.L.mskf_ekf_get_dim(self.h, C.byref(d)))
        return d.value

    def ekf_get_cov(self):
        d = self.ekf_dim()
        P = np.zeros((d, d))
        _chk(self.L.mskf_ekf_get_cov(self.h, _p(P), P.size))
        return P

    def ekf_debug_plane(self):
        """mskf_ekf_debug_read(which = 6): the whole current covariance plane, ld x ld doubles.  Only [0, d) x [0, d) is live;
        the rest is what earlier calls left there.  For tests."""
        ld = C.c_int()
        probe = np.zeros(1)
        self.L.mskf_ekf_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        _chk(self.L.mskf_ekf_debug_read(self.h, 6, _p(probe), probe.nbytes, C.byref(ld)))
        out = np.zeros((ld.value, ld.value))
        _chk(self.L.mskf_ekf_debug_read(self.h, 6, _p(out), out.nbytes, C.byref(ld)))
        return out

    def ekf_propagate(self, Phi, Q):
        Phi = np.ascontiguousarray(Phi, dtype=np.float64).reshape(-1, 21, 21)
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 21, 21)
        _chk(self.L.mskf_ekf_propagate(self.h, len(Phi), _p(Phi), _p(Q)))

    def ekf_augment(self, J):
        J = np.ascontiguousarray(J, dtype=np.float64)
        assert J.shape == (6, 21)
        _chk(self.L.mskf_ekf_augment(self.h, _p(J)))

    def ekf_remove_clone(self, idx):
        _chk(self.L.mskf_ekf_remove_clone(self.h, idx))

    def ekf_propagate_imu(self, steps):
        """mskf_ekf_propagate_imu over IMU_STEP records (Phi and Q are formed on the device)."""
        st = _imu_steps(steps)
        self.L.mskf_ekf_propagate_imu.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _chk(self.L.mskf_ekf_propagate_imu(self.h, len(st), st.ctypes.data if len(st) else None))

    def ekf_pos_var(self):
        out = np.full(3, np.nan)
        self.L.mskf_ekf_get_pos_var.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.mskf_ekf_get_pos_var(self.h, _p(out)))
        return out

    def ekf_odom_cov(self):
        """mskf_ekf_get_odom_cov: one ODOM_COV record (pose 6 x 6, twist 3 x 3, pos_var 3)."""
        out = np.zeros(1, ODOM_COV)
        out.view(np.float64)[:] = np.nan
        self.L.mskf_ekf_get_odom_cov.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self.L.mskf_ekf_get_odom_cov(self.h, _p(out)))
        return out[0]

    @staticmethod
    def _direct_args(stream, H=None, r=None, R=None, gate=0.0, pos_var=True):
        """(mskf_ekf_direct_args, buffers it points into, result dict the call fills) for one stream; no H: m = 0."""
        d = stream.ekf_dim()
        dx = np.zeros(d)
        pv = np.full(3, np.nan)
        a = EkfDirectArgs()
        a.status, a.gamma = -1, float("nan")
        keep = [dx, pv]
        if H is not None:
            r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
            m = len(r)
            H = np.ascontiguousarray(H, dtype=np.float64).reshape(m, 21)
            R = np.ascontiguousarray(R, dtype=np.float64).reshape(m, m)
            a.m, a.H, a.r, a.R = m, H.ctypes.data, r.ctypes.data, R.ctypes.data
            keep += [H, r, R]
        a.gate = float(gate)
        a.delta_x = dx.ctypes.data
        a.pos_var_out = pv.ctypes.data if pos_var else None
        return a, keep, dict(delta_x=dx, pos_var=pv, gamma=float("nan"), status=-1)

    def ekf_update_direct(self, H, r, R, gate=0.0, pos_var=True):
        """mskf_ekf_update_direct: H (m x 21, m <= 6) on the IMU block, residual r, covariance R, gate (> 0: applied only when
        gamma <= gate).  Returns dict(delta_x, gamma, status (1 applied, 0 gated out, 2 S not positive definite), pos_var)."""
        a, _keep, res = self._direct_args(self, H, r, R, gate, pos_var)
        self.L.mskf_ekf_update_direct.argtypes = [C.c_void_p, C.POINTER(EkfDirectArgs)]
        _chk(self.L.mskf_ekf_update_direct(self.h, C.byref(a)))
        res["gamma"], res["status"] = float(a.gamma), int(a.status)
        return res

    @staticmethod
    def _update_args(gravity, clones, positions, obs_start, obs_clone, obs_z, dof_offset, apply_row_cap, needs_init=None, init_ranges=None):
        """(mskf_ekf_update_args, buffers it points into, result builder) for one stream."""
        clones = np.ascontiguousarray(clones, dtype=np.float64).reshape(-1, 14)
        n_clones = len(clones)
        obs_start = np.asarray(obs_start, dtype=np.int32)
        n_feat = len(obs_start) - 1
        obs_clone = np.ascontiguousarray(obs_clone, dtype=np.int32)
        obs_z = np.ascontiguousarray(obs_z, dtype=np.float64).reshape(-1, 4)
        feats = np.zeros(n_feat, EKF_FEATURE)
        feats["obs_start"] = obs_start[:-1]
        feats["n_obs"] = np.diff(obs_start)
        if positions is not None:
            feats["position"] = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        if needs_init is not None:
            feats["needs_init"] = np.asarray(needs_init, dtype=np.int32)
            if init_ranges is None:
                feats["init_start"] = feats["obs_start"]
                feats["n_init"] = feats["n_obs"]
            else:
                feats["init_start"] = [r[0] for r in init_ranges]
                feats["n_init"] = [r[1] for r in init_ranges]
        d = 21 + 6 * n_clones
        dx = np.zeros(d)
        status = np.zeros(max(n_feat, 1), np.uint8)
        gamma = np.zeros(max(n_feat, 1))
        rows = np.zeros(1, np.int32)
        diag = np.zeros(2, np.int32)
        pos_var = np.full(3, np.nan)
        a = EkfUpdateArgs()
        a.n_clones, a.n_feat, a.n_obs = n_clones, n_feat, len(obs_clone)
        a.dof_offset, a.apply_row_cap = dof_offset, int(apply_row_cap)
        a.gravity[:] = list(np.asarray(gravity, dtype=np.float64))
        a.clones, a.features, a.obs_clone, a.obs_z = clones.ctypes.data, feats.ctypes.data, obs_clone.ctypes.data, obs_z.ctypes.data
        a.delta_x, a.feat_status, a.gamma, a.rows_out = dx.ctypes.data, status.ctypes.data, gamma.ctypes.data, rows.ctypes.data
        a.diag_out = diag.ctypes.data
        a.pos_var_out = pos_var.ctypes.data
        keep = (clones, feats, obs_clone, obs_z, dx, status, gamma, rows, diag, pos_var)

        def result():
            return dict(delta_x=dx, status=status[:n_feat], gamma=gamma[:n_feat], rows=int(rows[0]),
                        positions=feats["position"].copy(), used_qr=int(diag[0]), tiny_pivots=int(diag[1]),
                        pos_var=pos_var.copy())
        return a, keep, result

    def ekf_update(self, gravity, clones, positions, obs_start, obs_clone, obs_z, dof_offset, apply_row_cap,
                   needs_init=None, init_ranges=None):
        """clones: (n,14) [q p q_null p_null]; obs_start: n_feat+1 offsets; returns dict."""
        a, keep, result = self._update_args(gravity, clones, positions, obs_start, obs_clone, obs_z, dof_offset, apply_row_cap, needs_init, init_ranges)
        _chk(self.L.mskf_ekf_update(self.h, C.byref(a)))
        return result()
