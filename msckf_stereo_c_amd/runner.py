"""Python driver of the host mirror classes (cg::System / MultiRunner, csrc/host) — the product path.

Everything below the binding is C++ above the C-ABI and HIP kernels below it; nothing here computes.
"""
import ctypes as C
import os

import numpy as np

from .capi import MskfError
from .ctypes_types import (EQUALIZE_MODES, FEATURE_MEAS, INPUT_FORMATS, ODOM_COV, POINT2F, POSE, Calib, EkfCfg, FeCfg, FeEqualize, FeInputFormat, FeMask,
                           FB_CHECK_MODES, FeCameraModel, FeFbCheck, FePatchCheck, ImuSample, PATCH_CHECK_MODES, TrackingInfo, camera_model_cfg, raw_raster)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

IMU_SAMPLE = np.dtype([("t", "<f8"), ("w", "<f8", 3), ("a", "<f8", 3)])


def lib():
    global _LIB
    if _LIB is None:
        p = os.path.join(_HERE, "_build", "libmskf_host.so")
        if not os.path.exists(p):
            raise MskfError("libmskf_host.so is not built (run python -m msckf_stereo_c_amd.build); there is no CPU fallback")
        L = C.CDLL(p)
        L.mskfh_runner_create.restype = C.c_void_p
        L.mskfh_runner_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(Calib), C.POINTER(FeCfg), C.POINTER(EkfCfg), C.c_int, C.c_int]
        L.mskfh_runner_set_workers.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mskfh_runner_set_compression.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_destroy.argtypes = [C.c_void_p]
        L.mskfh_runner_error.restype = C.c_char_p
        L.mskfh_runner_error.argtypes = [C.c_void_p]
        L.mskfh_runner_imu.argtypes = [C.c_void_p, C.c_int, C.POINTER(ImuSample)]
        L.mskfh_runner_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_runner_set_sequence.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                                C.c_longlong, C.c_longlong, C.c_void_p, C.c_int]
        L.mskfh_runner_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mskfh_runner_keep_trajectory.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_keep_trajectory_stream.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mskfh_runner_publish_covariance.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mskfh_runner_set_equalize.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeEqualize)]
        L.mskfh_runner_set_input_format.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeInputFormat)]
        L.mskfh_runner_set_zupt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double]
        L.mskfh_runner_fuse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
        L.mskfh_num_odom_covs.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_num_odom_covs.restype = C.c_int
        L.mskfh_get_odom_covs.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_runner_run_timed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.mskfh_runner_frames_done.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_window.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_runner_get_window_phases.argtypes = [C.c_void_p, C.c_void_p]
        L.mskfh_runner_mark_dump_size.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_mark_dump.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.mskfh_runner_set_stagger.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_group_offset.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_group_offset.restype = C.c_int
        for name in ("mskfh_num_features", "mskfh_msg_size", "mskfh_num_poses", "mskfh_state_dim", "mskfh_num_updates",
                     "mskfh_num_clones", "mskfh_num_direct_updates", "mskfh_num_zupt"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_int]
            getattr(L, name).restype = C.c_int
        L.mskfh_num_tsqr_updates.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_num_tsqr_updates.restype = C.c_int
        L.mskfh_num_uncompressed_updates.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_num_uncompressed_updates.restype = C.c_int
        L.mskfh_stacked_rows.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_stacked_rows.restype = C.c_longlong
        L.mskfh_num_resets.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_num_resets.restype = C.c_longlong
        L.mskfh_num_device_frames.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_num_device_frames.restype = C.c_longlong
        L.mskfh_get_dump.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(TrackingInfo)]
        L.mskfh_get_msg.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_get_poses.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_get_cov.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.mskfh_get_imu_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mskfh_runner_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_runner_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mskfh_runner_get_phases.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mskfh_group_hip_stream.argtypes = [C.c_void_p, C.c_int]
        L.mskfh_group_hip_stream.restype = C.c_void_p
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pose_rotation(q):
    """R (3, 3) of a POSE record's q = (x, y, z, w): the rotation IMU -> world, p_w = R p_i + p.  The filter's own quaternion is the
    JPL one of world -> IMU (ekf_meas.h), which has the same four components."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def imu_position_from_verification(R, t, pose_k, calib):
    """The world position of the IMU at the query frame, which is what fuse_position takes, from a verified motion p_k = R p_q + t
    (query cam0 -> keyframe cam0: what verify_keyframes returns), the keyframe's published pose pose_k (the POSE record of
    Runner.poses at the keyframe's time: p, q) and calib.T_cam0_imu (p_c = R_ci p_i + t_ci; T_imu_body is taken as the identity):
        p_w = R_wi(q_k) R_ci^T (R t_ci + t - t_ci) + p_k        ("Geometric verification").
    The query IMU's origin is t_ci in the query's cam0, R t_ci + t in the keyframe's cam0, R_ci^T (. - t_ci) in the keyframe's IMU
    frame.  A pure function: it reads nothing of a runner."""
    T = np.array(calib.T_cam0_imu, np.float64).reshape(4, 4)
    R_ci, t_ci = T[:3, :3], T[:3, 3]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return pose_rotation(pose_k["q"]) @ (R_ci.T @ (R @ t_ci + t - t_ci)) + np.array(pose_k["p"], np.float64)


def set_fe_books_on_host(on):
    """Process-wide: 1 = the front-end's bookkeeping stays on the host for every frame (the phased mskf_fe_track path), 0 = whole
    frames on the device wherever the configuration allows (default), -1 = back to the MSKF_FE_BOOKS environment variable."""
    lib().mskfh_set_fe_books_on_host(int(on))


class Runner:
    """n_groups x per_group independent VIO streams on one GPU."""

    def __init__(self, calib, fe_cfg, ekf_cfg, n_groups=1, per_group=1, device=0, host_threads=1, ekf_host_threads=0):
        """host_threads / ekf_host_threads: threads sharing the per-stream host phases of a group's front-end / filter stage
        (0 = as host_threads)."""
        self.L = lib()
        self.calib, self.fe_cfg, self.ekf_cfg = calib, fe_cfg, ekf_cfg
        self.n = n_groups * per_group
        self.n_groups, self.per_group = n_groups, per_group
        self.h = self.L.mskfh_runner_create(device, n_groups, per_group, C.byref(calib), C.byref(fe_cfg), C.byref(ekf_cfg), host_threads, ekf_host_threads)
        if not self.h:
            raise MskfError("could not create the runner (no GPU / HIP library?): see stderr")
        self._keep = []
        self._fmt = [0] * self.n          # MSKF_PIX_* of every stream (set_input_format)

    def close(self):
        if self.h:
            self.L.mskfh_runner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MskfError("runner status %d: %s" % (rc, self.L.mskfh_runner_error(self.h).decode()))

    def set_compression(self, mode):
        """QR compression of every stream from its next update on: 0 auto, 1 Gram + Cholesky, 2 Householder TSQR (call between runs)."""
        self._chk(self.L.mskfh_runner_set_compression(self.h, int(mode)))

    def set_workers(self, fe_workers=0, ekf_workers=0):
        """Workers of the balanced runner (MultiRunner::run_balanced): front-end / filter workers that serve the n_groups
        batches; 0 = one of a kind per batch."""
        self.L.mskfh_runner_set_workers(self.h, int(fe_workers), int(ekf_workers))

    def imu(self, stream, sample):
        self.L.mskfh_runner_imu(self.h, stream, C.byref(sample))

    def step(self, cam0_list, cam1_list, times):
        """One frame for every stream from host images (numpy u8 arrays; with set_input_format, arrays of the format's dtype and
        shape: (h, w) uint16, (h, w, 3 | 4) uint8, (h, w) uint8 of the calibration's size)."""
        a = [np.ascontiguousarray(x, dtype=np.uint8) if f == 0 else self._raw(x, f) for x, f in zip(cam0_list, self._fmt)]
        b = [np.ascontiguousarray(x, dtype=np.uint8) if f == 0 else self._raw(x, f) for x, f in zip(cam1_list, self._fmt)]
        pa = (C.c_void_p * self.n)(*[x.ctypes.data for x in a])
        pb = (C.c_void_p * self.n)(*[x.ctypes.data for x in b])
        t = np.ascontiguousarray(times, dtype=np.float64)
        self._chk(self.L.mskfh_runner_step(self.h, pa, pb, 0, _p(t)))

    def set_sequence(self, stream, cam0_base_ptr, cam1_base_ptr, on_device, frame_bytes, n_static, n_loop, t0_ns, frame_dt_ns, imu):
        imu = np.ascontiguousarray(imu, dtype=IMU_SAMPLE)
        self._keep.append(imu)
        self.L.mskfh_runner_set_sequence(self.h, stream, cam0_base_ptr, cam1_base_ptr, int(on_device), frame_bytes, n_static, n_loop,
                                         t0_ns, frame_dt_ns, _p(imu), len(imu))

    def run(self, first, n, threaded=True, pipelined=False):
        """Frames [first, first+n) of the attached sequences.  pipelined: front-end and filter of every group run
        as a two-stage pipeline on two HIP streams (identical results: the front-end never reads filter state), all groups in
        one run of MultiRunner::run_balanced.  threaded applies to lockstep runs only: the groups on their own host threads
        (True) or one after another."""
        self._chk(self.L.mskfh_runner_run(self.h, first, n, int(threaded), int(pipelined)))

    def run_timed(self, first, warmup, steps, max_extra=8):
        """ONE pipelined run of every group over at least `warmup` + `steps` frames (no fill / drain of the group pipelines at
        the boundary).  Returns the seconds in which the groups together completed frames n_groups * warmup + 1 ..
        n_groups * (warmup + steps) of the run: exactly `steps` steps' worth of stream-frames, with every group busy from
        before that window opens until after it closes (MultiRunner::run_timed)."""
        el = C.c_double(0.0)
        self._chk(self.L.mskfh_runner_run_timed(self.h, first, warmup, steps, max_extra, C.byref(el)))
        return el.value

    def frames_done(self, group=0):
        """Next frame index of a group (absolute, its stagger offset included)."""
        return self.L.mskfh_runner_frames_done(self.h, group)

    def window(self, group=0):
        out = np.zeros(7)
        self.L.mskfh_runner_window(self.h, group, _p(out))
        return dict(zip(("fe_open", "fe_close", "ekf_open", "ekf_close", "fe_frames", "ekf_frames", "frames_at_close"), (float(x) for x in out)))

    def mark_dump(self, group=0):
        """(ids, lifetimes, cam0, cam1, imu_state[28]) of local stream 0 of a group at the close of its timed window."""
        n = self.L.mskfh_runner_mark_dump_size(self.h, group)
        if n < 0:
            raise MskfError("no timed window has been closed")
        ids = np.zeros(n, np.uint64)
        life = np.zeros(n, np.int32)
        c0 = np.zeros(n, POINT2F)
        c1 = np.zeros(n, POINT2F)
        imu = np.zeros(28)
        self.L.mskfh_runner_mark_dump(self.h, group, _p(ids), _p(life), _p(c0), _p(c1), _p(imu))
        return ids, life, c0, c1, imu

    def set_stagger(self, delta):
        """Group g works g * delta frames ahead of the index passed to run() (MultiRunner::set_stagger)."""
        self.L.mskfh_runner_set_stagger(self.h, int(delta))

    def group_offset(self, g):
        return self.L.mskfh_runner_group_offset(self.h, g)

    def keep_trajectory(self, keep, stream=None):
        if stream is None:
            self.L.mskfh_runner_keep_trajectory(self.h, int(keep))
        else:
            self.L.mskfh_runner_keep_trajectory_stream(self.h, int(stream), int(keep))

    def set_equalize(self, mode, tiles=(8, 8), clip_limit=40.0, stream=None):
        """Opt-in equalisation of the pushed images of one stream or of all (mskf_fe_set_equalize): mode "off" / 0, "hist" / 1
        (global histogram equalisation), "clahe" / 2 with tiles = (tiles_x, tiles_y) and clip_limit.  Call before the first frame."""
        cfg = FeEqualize(int(EQUALIZE_MODES.get(mode, mode)), int(tiles[0]), int(tiles[1]), 0, float(clip_limit))
        rc = self.L.mskfh_runner_set_equalize(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_mask(self, cam0=None, cam1=None, margin=0, stream=None):
        """Opt-in image masks of one stream or of all (mskf_fe_set_mask): (h, w) arrays in which a pixel != 0 is USABLE and 0 is
        masked out; None = that camera is not masked, both None = off.  margin (0 .. 64) erodes the usable set.  The detector
        records no masked-out cam0 pixel, tracked points that land on a masked-out pixel are dropped.  Call between runs."""
        planes = [None if m is None else np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8) for m in (cam0, cam1)]
        shapes = {m.shape for m in planes if m is not None}
        if len(shapes) > 1 or any(m.ndim != 2 for m in planes if m is not None):
            raise MskfError("the masks are 2-D planes of one size", -1)
        h, w = shapes.pop() if shapes else (0, 0)
        cfg = FeMask(None if planes[0] is None else planes[0].ctypes.data, None if planes[1] is None else planes[1].ctypes.data, w, h, w, int(margin))
        self.L.mskfh_runner_set_mask.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeMask)]
        rc = self.L.mskfh_runner_set_mask(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_patch_check(self, mode="both", half=4, min_zncc_temporal=0.8, min_zncc_stereo=0.8, stream=None):
        """Opt-in ZNCC patch check of one stream or of all (mskf_fe_set_patch_check): tracked points whose patch no longer
        correlates with the previous frame's ("temporal") and stereo matches whose patches do not correlate ("stereo") are dropped
        behind every track launch.  mode "both" / "temporal" / "stereo" / "off"; half 2 .. 7; thresholds in [0, 1].  Call between runs."""
        if isinstance(mode, str) and mode not in PATCH_CHECK_MODES:
            raise MskfError("unknown patch check mode %r" % (mode,), -1)
        cfg = FePatchCheck(int(PATCH_CHECK_MODES.get(mode, mode)), int(half), float(min_zncc_temporal), float(min_zncc_stereo))
        self.L.mskfh_runner_set_patch_check.argtypes = [C.c_void_p, C.c_int, C.POINTER(FePatchCheck)]
        rc = self.L.mskfh_runner_set_patch_check(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_fb_check(self, mode="both", max_error_temporal=1.0, max_error_stereo=1.0, stream=None):
        """Opt-in forward-backward check of one stream or of all (mskf_fe_set_fb_check): tracked points ("temporal") and stereo
        matches ("stereo") that LK, run backwards from the known origin, does not bring back to within the threshold are dropped
        behind every track launch.  mode "both" / "temporal" / "stereo" / "off"; thresholds in level-0 pixels, 0 .. 64.  Call
        between runs."""
        if isinstance(mode, str) and mode not in FB_CHECK_MODES:
            raise MskfError("unknown forward-backward check mode %r" % (mode,), -1)
        cfg = FeFbCheck(int(FB_CHECK_MODES.get(mode, mode)), float(max_error_temporal), float(max_error_stereo))
        self.L.mskfh_runner_set_fb_check.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeFbCheck)]
        rc = self.L.mskfh_runner_set_fb_check(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_lk_levels(self, levels, stream=None):
        """Opt-in deeper LK pyramids of one stream or of all (mskf_fe_set_lk_levels): every LK of the stream runs over `levels` = 4 .. 8
        pyramid levels (4: the default).  Deeper reaches further and is not better: see README.  Call before the first frame."""
        self.L.mskfh_runner_set_lk_levels.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.L.mskfh_runner_set_lk_levels(self.h, -1 if stream is None else int(stream), int(levels))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_camera_model(self, cam, model, coeffs, stream=None):
        """Opt-in camera model of camera `cam` (0 / 1) of one stream or of all (mskf_fe_set_camera_model): "radtan8" (OpenCV's 5 or 8
        coefficients k1 k2 p1 p2 k3 [k4 k5 k6]), "fov" (w), "ds" (xi, alpha), or "radtan" / "equidistant" with four coefficients,
        which put the camera back on the base path.  The intrinsics stay the calibration's.  Call between runs."""
        try:
            cfg = camera_model_cfg(cam, model, coeffs)
        except ValueError as e:
            raise MskfError(str(e), -1)
        self.L.mskfh_runner_set_camera_model.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeCameraModel)]
        rc = self.L.mskfh_runner_set_camera_model(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)

    def set_descriptors(self, on, stream=None):
        """Opt-in 256-bit binary descriptors (upright BRIEF) of the features every frame publishes, of one stream
        or of all: one more batched device call per frame of a group with a describing stream.  Off by default; call between runs."""
        self.L.mskfh_runner_set_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.L.mskfh_runner_set_descriptors(self.h, -1 if stream is None else int(stream), int(bool(on)))
        if rc != 0:
            raise MskfError("set_descriptors: the stream is not one of the runner's", rc)

    def descriptors(self, stream=0):
        """(ids uint64[n], desc uint8[n, 32], valid uint8[n]) of the stream's last frame, aligned with msg(stream): the descriptors
        of that frame's cam0 image at the cam0 pixels of its features.  Empty arrays with the option off."""
        self.L.mskfh_num_descriptors.argtypes = [C.c_void_p, C.c_int]
        self.L.mskfh_get_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        n = self.L.mskfh_num_descriptors(self.h, stream)
        ids, desc, valid = np.zeros(n, np.uint64), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        if n:
            self.L.mskfh_get_descriptors(self.h, stream, _p(ids), _p(desc), _p(valid))
        return ids, desc, valid

    def add_keyframe(self, stream=0):
        """Keep a copy of the stream's last-frame (time, ids, desc, valid), what descriptors(stream) returns, as a keyframe in host
        memory; returns its index.  The runner decides neither when a frame becomes a keyframe nor what counts as a revisit: that is
        the caller's policy.  Raises with descriptors off for the stream.  Call between runs."""
        self.L.mskfh_add_keyframe.argtypes = [C.c_void_p, C.c_int]
        k = self.L.mskfh_add_keyframe(self.h, int(stream))
        if k < 0:
            raise MskfError("add_keyframe: descriptors are off for the stream (set_descriptors), or it is not one of the runner's", -1)
        return k

    def num_keyframes(self, stream=0):
        self.L.mskfh_num_keyframes.argtypes = [C.c_void_p, C.c_int]
        return self.L.mskfh_num_keyframes(self.h, int(stream))

    def keyframe(self, stream, k):
        """(time, ids uint64[n], desc uint8[n, 32], valid uint8[n]) of the stream's keyframe k."""
        self.L.mskfh_keyframe_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.L.mskfh_get_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
        n = self.L.mskfh_keyframe_size(self.h, int(stream), int(k))
        if n < 0:
            raise IndexError("keyframe %d of stream %d" % (k, stream))
        t = C.c_double(0)
        ids, desc, valid = np.zeros(n, np.uint64), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        self.L.mskfh_get_keyframe(self.h, int(stream), int(k), C.byref(t), _p(ids), _p(desc), _p(valid))
        return t.value, ids, desc, valid

    def clear_keyframes(self, stream=None):
        """Forget the keyframes of one stream, or of all."""
        self.L.mskfh_clear_keyframes.argtypes = [C.c_void_p, C.c_int]
        self.L.mskfh_clear_keyframes(self.h, -1 if stream is None else int(stream))

    def query_keyframes(self, stream=0, max_distance=256, ratio=0.0, cross_check=True, min_matches=0):
        """Match the stream's last-frame descriptors against every keyframe of that stream in one mskf_fe_match_batch (the query set
        is shared, one job per keyframe; DESIGN.md section 3, "Descriptor matching").  Returns [(k, time, n_matches, pairs)] of the
        keyframes with n_matches >= min_matches, pairs uint64[m, 2] of (query feature id, keyframe feature id) in query order.
        verify_keyframes checks the hits geometrically; deciding on a candidate and fusing it (fuse_position) stay with the caller.
        Call between runs."""
        self.L.mskfh_query_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]
        self.L.mskfh_keyframe_hit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p]
        n = self.L.mskfh_query_keyframes(self.h, int(stream), int(max_distance), float(ratio), int(bool(cross_check)), int(min_matches))
        if n < 0:
            from . import capi
            raise MskfError("query_keyframes: mskf status %d: %s" % (n, capi.lib().mskf_last_error().decode()), n)
        out = []
        for i in range(n):
            k, t, m = C.c_int(0), C.c_double(0), C.c_int(0)
            self.L.mskfh_keyframe_hit(self.h, int(stream), i, C.byref(k), C.byref(t), C.byref(m), None)
            pairs = np.zeros((m.value, 2), np.uint64)
            self.L.mskfh_keyframe_hit(self.h, int(stream), i, C.byref(k), C.byref(t), C.byref(m), _p(pairs))
            out.append((k.value, t.value, m.value, pairs))
        return out

    def keyframe_obs(self, stream, k):
        """float64[n, 4] of the stream's keyframe k: x0, y0, x1, y1 per feature, the undistorted normalised stereo coordinates the
        keyframe's frame published (u0, v0, u1, v1 of msg) for the features of keyframe(stream, k), in their order."""
        self.L.mskfh_keyframe_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.L.mskfh_get_keyframe_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        n = self.L.mskfh_keyframe_size(self.h, int(stream), int(k))
        if n < 0:
            raise IndexError("keyframe %d of stream %d" % (k, stream))
        obs = np.zeros((n, 4), np.float64)
        self.L.mskfh_get_keyframe_obs(self.h, int(stream), int(k), _p(obs))
        return obs

    def verify_keyframes(self, stream=0, n_hypotheses=256, max_error=None, min_depth=0.1, max_depth=40.0, min_inliers=12, seed=0):
        """The stereo RANSAC pose check ("Geometric verification") of every hit of the stream's last
        query_keyframes, in one mskf_fe_verify_batch: a job per hit, its pairs the hit's matches as (the last frame's, the keyframe's)
        stereo observations.  max_error is in normalised units, None = 2 px over cam0's fx; that, min_depth = 0.1 m and max_depth =
        40 m are untuned starting values.  Returns [(k, time, n_matches, n_inliers, R, t, info, rms, inlier_pairs)] of the hits with
        status 0 and n_inliers >= min_inliers: p_keyframe = R p_query + t in cam0 coordinates (imu_position_from_verification turns
        that into what fuse_position takes), info (6, 6) = J^T J in the order [theta, t] (a covariance is sigma^2 info^-1), rms of the
        residuals, inlier_pairs uint64[n_inliers, 2] the (query feature id, keyframe feature id) of the inliers.  min_inliers is this
        method's filter, not the ABI's.  Raises when a newer frame has been described since the query: the hits are then not this
        frame's.  The runner still decides nothing about keyframe policy and never calls fuse_position itself.  Call between runs."""
        if max_error is None:
            max_error = 2.0 / float(self.calib.cam0_intrinsics[0])
        self.L.mskfh_verify_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double]
        self.L.mskfh_keyframe_verification.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.mskfh_verify_refused.argtypes = [C.c_void_p, C.c_int]
        self.L.mskfh_verify_refused.restype = C.c_char_p
        n = self.L.mskfh_verify_keyframes(self.h, int(stream), int(n_hypotheses), int(seed) & 0xFFFFFFFFFFFFFFFF, float(max_error), float(min_depth), float(max_depth))
        if n < 0:
            from . import capi
            why = self.L.mskfh_verify_refused(self.h, int(stream)).decode() if 0 <= int(stream) < self.n else ""
            raise MskfError("verify_keyframes: mskf status %d: %s" % (n, why or capi.lib().mskf_last_error().decode()), n)
        self.L.mskfh_keyframe_hit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p]
        out = []
        for i in range(n):
            ints, dbl = np.zeros(6, np.int32), np.zeros(50, np.float64)
            self.L.mskfh_keyframe_verification(self.h, int(stream), i, _p(ints), _p(dbl), None)
            k, n_matches, _n_usable, n_inliers, _best, status = (int(v) for v in ints)
            inl = np.zeros(max(n_matches, 1), np.uint8)
            self.L.mskfh_keyframe_verification(self.h, int(stream), i, _p(ints), _p(dbl), _p(inl))
            if status != 0 or n_inliers < min_inliers:
                continue
            hk, ht, hm = C.c_int(0), C.c_double(0), C.c_int(0)
            pairs = np.zeros((n_matches, 2), np.uint64)          # record i belongs to hit i of the query
            self.L.mskfh_keyframe_hit(self.h, int(stream), i, C.byref(hk), C.byref(ht), C.byref(hm), _p(pairs))
            assert (hk.value, hm.value) == (k, n_matches)
            out.append((k, float(dbl[0]), n_matches, n_inliers, dbl[2:11].reshape(3, 3).copy(), dbl[11:14].copy(), dbl[14:50].reshape(6, 6).copy(), float(dbl[1]),
                        pairs[inl[:n_matches] != 0].copy()))
        return out

    def _raw(self, img, fmt):
        r = raw_raster(img, fmt)
        if r.shape[:2] != (self.calib.height, self.calib.width):
            raise ValueError("image of %d x %d for a calibration of %d x %d" % (r.shape[1], r.shape[0], self.calib.width, self.calib.height))
        return r

    def set_input_format(self, fmt, shift=0, stream=None):
        """Pixel format of the images of one stream or of all (mskf_fe_set_input_format): "gray8" (default), "gray16" with shift 0 .. 8
        (g = min(v >> shift, 255)), "rgb8", "bgr8", "rgba8", "bgra8", "bayer_rggb8" / "_grbg8" / "_gbrg8" / "_bggr8" (the name spells
        the top-left 2 x 2 tile), or the number.  The images are converted to 8-bit grey on the device inside the push.  step() then
        takes arrays of the format's dtype and shape; a sequence (set_sequence) holds raw frames of frame_bytes = w * h * bytes per
        pixel.  Call before the first frame."""
        if isinstance(fmt, str) and fmt not in INPUT_FORMATS:
            raise MskfError("unknown input format %r" % (fmt,), -1)
        cfg = FeInputFormat(int(INPUT_FORMATS.get(fmt, fmt)), int(shift))
        rc = self.L.mskfh_runner_set_input_format(self.h, -1 if stream is None else int(stream), C.byref(cfg))
        if rc != 0:
            from . import capi
            raise MskfError("mskf status %d: %s" % (rc, capi.lib().mskf_last_error().decode()), rc)
        for i in range(self.n):
            if stream is None or i == int(stream):
                self._fmt[i] = cfg.format

    def publish_covariance(self, on, stream=None):
        """MsckfVio::publishCovariance of one stream or of all: every published pose gets its 6 x 6 pose and 3 x 3 velocity
        covariance (one device read-out per filter frame).  Off by default; set it before the first frame."""
        self.L.mskfh_runner_publish_covariance(self.h, -1 if stream is None else int(stream), int(on))

    def set_zupt(self, on, max_disparity=0.5, min_features=20, noise_std=0.05, stream=None):
        """Opt-in zero-velocity update of one stream or of all: a frame whose message has at least min_features cam0 points in common
        with the previous message, moved by less than max_disparity pixels on average, fuses velocity = 0 with standard deviation
        noise_std (m/s), gated.  The defaults are starting values nobody has tuned.  Call between runs."""
        rc = self.L.mskfh_runner_set_zupt(self.h, -1 if stream is None else int(stream), int(bool(on)), float(max_disparity), int(min_features), float(noise_std))
        if rc != 0:
            raise MskfError("set_zupt: max_disparity and noise_std must be positive, min_features not negative, the stream one of the runner's", rc)

    def _fuse(self, kind, stream, t, z, cov, gated):
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(3)
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(3, 3)
        rc = self.L.mskfh_runner_fuse(self.h, int(stream), kind, float(t), _p(z), _p(cov), int(bool(gated)))
        if rc != 0:
            raise MskfError("a fused measurement takes finite values and a symmetric covariance with a positive diagonal", rc)

    def fuse_velocity(self, stream, t, v, cov, gated=True):
        """Queue a world-frame measurement v (3) of the IMU's velocity with covariance cov (3 x 3) for the first filter frame of the
        stream whose time stamp is >= t; gated: applied only inside the 95 % chi-square gate of 3 degrees of freedom."""
        self._fuse(0, stream, t, v, cov, gated)

    def fuse_position(self, stream, t, p, cov, gated=True):
        """The same for a world-frame measurement p of the IMU's position."""
        self._fuse(1, stream, t, p, cov, gated)

    def num_direct_updates(self, stream=0):
        """Direct measurement updates applied to the stream (fused velocities and positions, zero-velocity updates)."""
        return self.L.mskfh_num_direct_updates(self.h, stream)

    def num_zupt(self, stream=0):
        """... of which zero-velocity updates."""
        return self.L.mskfh_num_zupt(self.h, stream)

    # indexed like the MSKF_K_* kinds of mskf_hip.h; "k_ekf_augment" keeps its place: the augmentation is fused into k_ekf_propagate, and
    # the slot counts the launches of k_ekf_direct_update (mskf_hip.h)
    KERNELS = ["k_pyr_down", "k_detect_cells", "k_track4", "k_ekf_propagate", "k_ekf_augment", "k_ekf_feature_blocks",
               "k_ekf_tsqr", "k_ekf_gemm", "k_ekf_chol_lds", "k_ekf_trsm", "k_ekf_small", "k_ekf_remove_clone", "k_pt_geom", "k_fe_book"]

    def set_timing(self, enable):
        self.L.mskfh_runner_set_timing(self.h, int(enable))

    def get_timing(self, reset=True):
        """Per-kernel HIP-event timing accumulated on the groups' own streams: {kernel: (ms, launches, units)}.  The key
        "k_ekf_augment" carries the launches of k_ekf_direct_update (fused measurements, zero-velocity updates; units: streams with
        rows) and nothing else: the augmentation itself runs inside k_ekf_propagate, and the slot keeps its name for the ABI.
        Likewise "k_pt_geom" carries the point gates behind a track launch (k_mask_points, k_patch_points, k_fb_points; units: streams)."""
        k = len(self.KERNELS)
        ms = np.zeros(k)
        launches = np.zeros(k, np.int64)
        units = np.zeros(k, np.int64)
        self.L.mskfh_runner_get_timing(self.h, _p(ms), _p(launches), _p(units), int(reset))
        return {n: (float(ms[i]), int(launches[i]), int(units[i])) for i, n in enumerate(self.KERNELS)}

    PHASES = ["push", "fe_prepare1", "track1", "fe_after1", "track2", "fe_after2", "ekf_A", "update1", "ekf_B", "update2",
              "ekf_C", "posvar", "imu_feed", "handoff", "fe_queue_wait", "ekf_queue_wait", "imu_feed_ekf", "direct"]
    FE_THREAD_PHASES = ["imu_feed", "push", "fe_prepare1", "track1", "fe_after1", "track2", "fe_after2", "handoff", "fe_queue_wait"]
    EKF_THREAD_PHASES = ["ekf_queue_wait", "imu_feed_ekf", "ekf_A", "update1", "ekf_B", "update2", "ekf_C", "posvar", "direct"]

    def get_window_phases_group(self, g):
        """The same for one group."""
        out = np.zeros(len(self.PHASES))
        self.L.mskfh_runner_get_window_phases_group.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.L.mskfh_runner_get_window_phases_group(self.h, int(g), _p(out))
        return {n: float(out[i]) for i, n in enumerate(self.PHASES)}

    def get_window_phases(self):
        """Wall seconds per phase inside the last timed window, summed over groups."""
        out = np.zeros(len(self.PHASES))
        self.L.mskfh_runner_get_window_phases(self.h, _p(out))
        return {n: float(out[i]) for i, n in enumerate(self.PHASES)}

    def get_phases(self, reset=True):
        """Wall seconds per BatchGroup::step phase, summed over groups (host bookkeeping vs device calls)."""
        out = np.zeros(len(self.PHASES))
        self.L.mskfh_runner_get_phases(self.h, _p(out), int(reset))
        return {n: float(out[i]) for i, n in enumerate(self.PHASES)}

    def get_abi_host_time(self, reset=True):
        """Host seconds inside the batched C-ABI calls, outside the device waits, summed over groups."""
        out = np.zeros(4)
        self.L.mskfh_runner_get_abi_host_time.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.L.mskfh_runner_get_abi_host_time(self.h, _p(out), int(reset))
        return dict(zip(("update_pack", "update_unpack", "track_pack", "track_unpack"), (float(x) for x in out)))

    def get_hostprof(self, reset=True):
        """Seconds of host bookkeeping per slot of csrc/host/host_prof.h, summed over all streams and threads."""
        out = np.zeros(64)
        self.L.mskfh_get_hostprof.restype = C.c_int
        self.L.mskfh_hostprof_name.restype = C.c_char_p
        n = self.L.mskfh_get_hostprof(_p(out), 64, int(reset))
        return {self.L.mskfh_hostprof_name(i).decode(): float(out[i]) for i in range(n)}

    def hip_stream(self, stream=0):
        return self.L.mskfh_group_hip_stream(self.h, stream)

    # ---- inspection
    def dump(self, stream=0):
        n = self.L.mskfh_num_features(self.h, stream)
        ids = np.zeros(n, np.uint64)
        life = np.zeros(n, np.int32)
        c0 = np.zeros(n, POINT2F)
        c1 = np.zeros(n, POINT2F)
        info = TrackingInfo()
        self.L.mskfh_get_dump(self.h, stream, _p(ids), _p(life), _p(c0), _p(c1), C.byref(info))
        return ids, life, c0, c1, info

    def msg(self, stream=0):
        n = self.L.mskfh_msg_size(self.h, stream)
        out = np.zeros(n, FEATURE_MEAS)
        if n:
            self.L.mskfh_get_msg(self.h, stream, _p(out))
        return out

    def poses(self, stream=0):
        n = self.L.mskfh_num_poses(self.h, stream)
        out = np.zeros(n, POSE)
        if n:
            self.L.mskfh_get_poses(self.h, stream, _p(out))
        return out

    def odom_cov(self, stream=0):
        """ODOM_COV records aligned with poses(stream); empty unless publish_covariance is on."""
        n = self.L.mskfh_num_odom_covs(self.h, stream)
        out = np.zeros(n, ODOM_COV)
        if n:
            self.L.mskfh_get_odom_covs(self.h, stream, _p(out))
        return out

    def cov(self, stream=0):
        d = self.L.mskfh_state_dim(self.h, stream)
        P = np.zeros((d, d))
        self._chk(self.L.mskfh_get_cov(self.h, stream, _p(P), P.size))
        return P

    def imu_state(self, stream=0):
        out = np.zeros(28)
        self.L.mskfh_get_imu_state(self.h, stream, _p(out))
        return out

    def num_updates(self, stream=0):
        return self.L.mskfh_num_updates(self.h, stream)

    def num_device_frames(self, stream=0):
        """Front-end frames of the stream that ran as ONE device call (mskf_fe_frame_batch_*), books and RANSAC included."""
        return int(self.L.mskfh_num_device_frames(self.h, stream))

    def num_tsqr_updates(self, stream=0):
        """Updates of the stream whose QR compression ran as Householder TSQR (the rest: Gram + Cholesky)."""
        return self.L.mskfh_num_tsqr_updates(self.h, stream)

    def num_uncompressed_updates(self, stream=0):
        """Updates whose stack had no more rows than active columns and was used as it is (msckf_vio.cpp:818-821)."""
        return self.L.mskfh_num_uncompressed_updates(self.h, stream)

    def stacked_rows(self, stream=0):
        return self.L.mskfh_stacked_rows(self.h, stream)

    def num_resets(self, stream=0):
        return self.L.mskfh_num_resets(self.h, stream)

    def num_clones(self, stream=0):
        return self.L.mskfh_num_clones(self.h, stream)


class StreamView:
    """Adapter so that oracle_py.Synth.feed() can drive one stream of a Runner with the reference
    harness call order (imu_callback xN, stereo_callback, backend_callback)."""

    def __init__(self, runner):
        assert runner.n == 1
        self.r = runner
        self._pending = None

    def imu(self, s):
        self.r.imu(0, s)

    def stereo(self, cam0, cam1, t):
        self._pending = (cam0, cam1, t)

    def backend(self):
        cam0, cam1, t = self._pending
        self.r.step([cam0], [cam1], [t])
