// host_capi.cpp — C entry points over the host mirror classes (cg::System, MultiRunner) for the Python
// tests and bench.py.  This is host glue above the C-ABI of include/mskf_hip.h, not part of it.
#include <cstring>
#include <string>
#include <vector>
#include "batch_runner.h"
#include "host_prof.h"

using namespace cg;

// An ImageProcessor setter on one stream of the runner, or on all (stream < 0), in stream order: the first status that is not
// MSKF_OK ends the call and is returned; the streams before it keep what they were given.
template <typename Set>
static int set_on_streams(void *h, int stream, Set set) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream >= r->n_streams()) return MSKF_ERR_INVALID;
    for (int i = 0; i < r->n_streams(); ++i)
        if (stream < 0 || i == stream) { const int rc = set(*r->system(i).imgproc_ptr_); if (rc != MSKF_OK) return rc; }
    return MSKF_OK;
}

extern "C" {

void *mskfh_runner_create(int device, int n_groups, int per_group, const mskf_calib *calib, const mskf_fe_cfg *fe, const mskf_ekf_cfg *ekf,
                          int host_threads, int ekf_host_threads) {
    MultiRunner *r = new MultiRunner(device, n_groups, per_group, *calib, *fe, *ekf, host_threads, ekf_host_threads);
    if (!r->ok()) {
        std::fprintf(stderr, "mskfh_runner_create: %s\n", r->error().c_str());
        delete r;
        return nullptr;
    }
    return r;
}
// parse the three YAML files the reference reads (Q16 paths relative to config_dir); 0 on success
int mskfh_load_configs(const char *config_dir, mskf_calib *calib, mskf_fe_cfg *fe, mskf_ekf_cfg *ekf) {
    try {
        const std::string d(config_dir);
        *calib = calib_from_yaml(YAML::LoadFile(d + "/camchain-imucam-euroc.yaml"));
        *fe = fe_cfg_from_yaml(YAML::LoadFile(d + "/app_imgproc.yaml"));
        *ekf = ekf_cfg_from_yaml(YAML::LoadFile(d + "/app_msckfvio.yaml"));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mskfh_load_configs: %s\n", e.what());
        return -1;
    }
}

// the optional zupt keys of an app_msckfvio.yaml (zupt_cfg_from_yaml); 0 on success
int mskfh_load_zupt_config(const char *yaml_path, int *on, double *max_disparity, int *min_features, double *noise_std) {
    try {
        const zupt::Config c = zupt_cfg_from_yaml(YAML::LoadFile(yaml_path));
        *on = c.on ? 1 : 0; *max_disparity = c.max_disparity; *min_features = c.min_features; *noise_std = c.noise_std;
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mskfh_load_zupt_config: %s\n", e.what());
        return -1;
    }
}

// where the front-end's bookkeeping runs (ImageProcessor::setFeBooksOnHost): tests compare the two paths
void mskfh_set_fe_books_on_host(int on) { ImageProcessor::setFeBooksOnHost(on); }
void mskfh_runner_destroy(void *h) { delete (MultiRunner *)h; }
int mskfh_runner_num_streams(void *h) { return ((MultiRunner *)h)->n_streams(); }
const char *mskfh_runner_error(void *h) { static thread_local std::string e; e = ((MultiRunner *)h)->error(); return e.c_str(); }

void mskfh_runner_imu(void *h, int stream, const mskf_imu_sample *s) { ((MultiRunner *)h)->imu(stream, *s); }
int mskfh_runner_step(void *h, const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, const double *t) {
    return ((MultiRunner *)h)->step(cam0, cam1, on_device, t);
}
void mskfh_runner_set_sequence(void *h, int stream, const uint8_t *cam0_base, const uint8_t *cam1_base, int on_device, size_t frame_bytes,
                               int n_static, int n_loop, long long t0_ns, long long frame_dt_ns, const mskf_imu_sample *imu, int n_imu) {
    StreamSequence &q = ((MultiRunner *)h)->sequence(stream);
    q.cam0_base = cam0_base; q.cam1_base = cam1_base; q.on_device = on_device; q.frame_bytes = frame_bytes;
    q.n_static = n_static; q.n_loop = n_loop; q.t0_ns = t0_ns; q.frame_dt_ns = frame_dt_ns; q.imu = imu; q.n_imu = n_imu;
    q.imu_cursor = 0;
}
// pipelined: front-end and filter of each group run as a two-stage pipeline (MultiRunner::run_balanced); threaded: the groups
// of a lockstep run on one host thread each
int mskfh_runner_run(void *h, int first, int n, int threaded, int pipelined) { return ((MultiRunner *)h)->run(first, n, threaded != 0, pipelined != 0); }
// `warmup` + `steps` frames of every group in one pipelined run; *elapsed_s covers exactly the `steps` frames (MultiRunner::run_timed)
int mskfh_runner_run_timed(void *h, int first, int warmup, int steps, int max_extra, double *elapsed_s) {
    return ((MultiRunner *)h)->run_timed(first, warmup, steps, max_extra, elapsed_s);
}
int mskfh_runner_frames_done(void *h, int g) { return ((MultiRunner *)h)->frames_done(g); }
// group g's stages in the last timed window: [0] front-end open, [1] front-end close, [2] filter open, [3] filter close (steady
// clock, s), [4] frames the front-end started inside, [5] frames the filter started inside, [6] frames of the run the batch had
// completed when the shared window closed
void mskfh_runner_window(void *h, int g, double out[7]) {
    const TimedWindow &w = ((MultiRunner *)h)->window(g);
    out[0] = w.t_fe_begin; out[1] = w.t_fe_end; out[2] = w.t_ekf_begin; out[3] = w.t_ekf_end; out[4] = w.fe_frames; out[5] = w.ekf_frames;
    out[6] = w.frames_at_close;
}
// wall seconds per phase inside the last timed window, summed over groups (each stage between its own marks)
void mskfh_runner_get_window_phases(void *h, double *out) {
    MultiRunner *r = (MultiRunner *)h;
    for (int k = 0; k < PH_COUNT; ++k) out[k] = 0;
    for (int g = 0; g < r->n_groups(); ++g)
        for (int k = 0; k < PH_COUNT; ++k) out[k] += r->group(g).window_phase_s[k];
}
void mskfh_runner_get_window_phases_group(void *h, int g, double *out) {
    MultiRunner *r = (MultiRunner *)h;
    for (int k = 0; k < PH_COUNT; ++k) out[k] = r->group(g).window_phase_s[k];
}
// state of local stream 0 of group g when its stages closed the window; returns the feature count (-1: no window closed)
int mskfh_runner_mark_dump_size(void *h, int g) {
    const BatchGroup::MarkDump &m = ((MultiRunner *)h)->group(g).mark_dump;
    return (m.fe_valid && m.ekf_valid) ? (int)m.ids.size() : -1;
}
void mskfh_runner_mark_dump(void *h, int g, uint64_t *ids, int32_t *lifetime, mskf_point2f *cam0, mskf_point2f *cam1, double *imu28) {
    const BatchGroup::MarkDump &m = ((MultiRunner *)h)->group(g).mark_dump;
    for (size_t i = 0; i < m.ids.size(); ++i) {
        ids[i] = m.ids[i]; lifetime[i] = m.life[i];
        cam0[i] = mskf_point2f{m.c0[i].x, m.c0[i].y}; cam1[i] = mskf_point2f{m.c1[i].x, m.c1[i].y};
    }
    std::memcpy(imu28, m.imu, sizeof(m.imu));
}
void mskfh_runner_keep_trajectory_stream(void *h, int stream, int keep) { ((MultiRunner *)h)->system(stream).msckfvio_ptr()->keepTrajectory = keep != 0; }
void mskfh_runner_set_stagger(void *h, int delta) { ((MultiRunner *)h)->set_stagger(delta); }
// QR compression of every stream's stacked Jacobian from the next update on (mskf_ekf_set_compression_mode); call between runs
int mskfh_runner_set_compression(void *h, int mode) {
    MultiRunner *r = (MultiRunner *)h;
    for (int i = 0; i < r->n_streams(); ++i) { const int rc = mskf_ekf_set_compression_mode(r->system(i).stream(), mode); if (rc != MSKF_OK) return rc; }
    return MSKF_OK;
}
void mskfh_runner_set_workers(void *h, int fe_workers, int ekf_workers) { ((MultiRunner *)h)->set_workers(fe_workers, ekf_workers); }
int mskfh_runner_group_offset(void *h, int g) { return ((MultiRunner *)h)->group_offset(g); }
void mskfh_runner_keep_trajectory(void *h, int keep) {
    MultiRunner *r = (MultiRunner *)h;
    for (int i = 0; i < r->n_streams(); ++i) r->system(i).msckfvio_ptr()->keepTrajectory = keep != 0;
}

void mskfh_runner_set_timing(void *h, int enable) {
    MultiRunner *r = (MultiRunner *)h;
    for (int g = 0; g < r->n_groups(); ++g) { mskf_ctx_set_timing(r->group(g).ctx(), enable); mskf_ctx_set_timing(r->group(g).ekf_ctx(), enable); }
}
// sums over groups; arrays of MSKF_K_COUNT
void mskfh_runner_get_timing(void *h, double *ms, long long *launches, long long *units, int reset) {
    MultiRunner *r = (MultiRunner *)h;
    for (int k = 0; k < MSKF_K_COUNT; ++k) { ms[k] = 0; launches[k] = 0; units[k] = 0; }
    for (int g = 0; g < r->n_groups(); ++g)
        for (mskf_ctx *c : {r->group(g).ctx(), r->group(g).ekf_ctx()}) {
            double m[MSKF_K_COUNT]; long long l[MSKF_K_COUNT], u[MSKF_K_COUNT];
            if (mskf_ctx_get_timing(c, m, l, u, reset) != MSKF_OK) continue;
            for (int k = 0; k < MSKF_K_COUNT; ++k) { ms[k] += m[k]; launches[k] += l[k]; units[k] += u[k]; }
        }
}

// host seconds inside the batched C-ABI calls (packing / unpacking around the device work), summed over groups:
// [0] update pack, [1] update unpack, [2] track pack, [3] track unpack
void mskfh_runner_get_abi_host_time(void *h, double *out, int reset) {
    MultiRunner *r = (MultiRunner *)h;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    for (int g = 0; g < r->n_groups(); ++g)
        for (mskf_ctx *c : {r->group(g).ctx(), r->group(g).ekf_ctx()}) { double t[4]; if (mskf_ctx_get_host_time(c, t, reset) == MSKF_OK) for (int k = 0; k < 4; ++k) out[k] += t[k]; }
}

// wall seconds per step() phase summed over groups (PH_*), optionally reset
void mskfh_runner_get_phases(void *h, double *out, int reset) {
    MultiRunner *r = (MultiRunner *)h;
    for (int k = 0; k < PH_COUNT; ++k) out[k] = 0;
    for (int g = 0; g < r->n_groups(); ++g)
        for (int k = 0; k < PH_COUNT; ++k) { out[k] += r->group(g).phase_s[k]; if (reset) r->group(g).phase_s[k] = 0; }
}

// host bookkeeping accounting (host_prof.h): seconds per slot summed over all streams/threads; returns the slot count
int mskfh_get_hostprof(double *out, int capacity, int reset) {
    for (int k = 0; k < cg::hostprof::N_SLOTS && k < capacity; ++k) {
        out[k] = (double)cg::hostprof::counters()[k].load() * 1e-9;
        if (reset) cg::hostprof::counters()[k].store(0);
    }
    return cg::hostprof::N_SLOTS;
}
const char *mskfh_hostprof_name(int slot) { return cg::hostprof::name(slot); }

// ---- per-stream inspection
// ImageProcessor::twoPointRansac on undistorted point pairs (host arithmetic only, no device involved)
void mskfh_two_point_ransac(int n, const mskf_point2f *pts1_und, const mskf_point2f *pts2_und, const double *R_p_c, const double *intrinsics,
                            double inlier_error, double success_probability, unsigned long long *draws, int32_t *markers) {
    std::vector<cg::Point2f> a(n), b(n);
    for (int i = 0; i < n; ++i) { a[i] = cg::Point2f(pts1_und[i].x, pts1_und[i].y); b[i] = cg::Point2f(pts2_und[i].x, pts2_und[i].y); }
    hm::Mat3 R;
    for (int i = 0; i < 9; ++i) R.m[i] = R_p_c[i];
    std::vector<int> m;
    cg::two_point_ransac(a, b, R, intrinsics, inlier_error, success_probability, *draws, m);
    for (int i = 0; i < n; ++i) markers[i] = m[i];
}

int mskfh_num_features(void *h, int stream) {
    std::vector<ImageProcessor::FeatureIDType> ids; std::vector<int> life; std::vector<Point2f> a, b;
    ((MultiRunner *)h)->system(stream).imgproc_ptr_->dumpCurrent(ids, life, a, b);
    return (int)ids.size();
}
void mskfh_get_dump(void *h, int stream, uint64_t *ids, int32_t *lifetime, mskf_point2f *cam0, mskf_point2f *cam1, mskf_tracking_info *info) {
    std::vector<ImageProcessor::FeatureIDType> id; std::vector<int> life; std::vector<Point2f> a, b;
    ImageProcessor &ip = *((MultiRunner *)h)->system(stream).imgproc_ptr_;
    ip.dumpCurrent(id, life, a, b);
    for (size_t i = 0; i < id.size(); ++i) {
        ids[i] = id[i]; lifetime[i] = life[i];
        cam0[i] = mskf_point2f{a[i].x, a[i].y}; cam1[i] = mskf_point2f{b[i].x, b[i].y};
    }
    info->time_stamp = ip.last_tracking_info.time_stamp;
    info->before_tracking = ip.last_tracking_info.before_tracking; info->after_tracking = ip.last_tracking_info.after_tracking;
    info->after_matching = ip.last_tracking_info.after_matching; info->after_ransac = ip.last_tracking_info.after_ransac;
}
// the message as the reference holds it: with the whole Q1 tail of never-written records (kept as a count by the batch runner)
int mskfh_msg_size(void *h, int stream) { return (int)((MultiRunner *)h)->system(stream).imgproc_ptr_->messageSize(); }
void mskfh_get_msg(void *h, int stream, mskf_feature_meas *out) {
    const ImageProcessor &ip = *((MultiRunner *)h)->system(stream).imgproc_ptr_;
    const auto &f = ip.feature_msg_ptr_->features;
    static_assert(sizeof(FeatureMeasurement) == sizeof(mskf_feature_meas), "record layout");
    std::memset(out, 0, ip.messageSize() * sizeof(mskf_feature_meas));
    std::memcpy(out, f.data(), f.size() * sizeof(mskf_feature_meas));
}
int mskfh_num_poses(void *h, int stream) { return (int)((MultiRunner *)h)->system(stream).msckfvio_ptr()->poses().size(); }
void mskfh_get_poses(void *h, int stream, mskf_pose *out) {
    const auto &p = ((MultiRunner *)h)->system(stream).msckfvio_ptr()->poses();
    std::memcpy(out, p.data(), p.size() * sizeof(mskf_pose));
}
// ImageProcessor::setEqualize (mskf_fe_set_equalize) of one stream, or of all (stream < 0); call before the first frame.
// Returns the first status that is not MSKF_OK (mskf_last_error has the text).
int mskfh_runner_set_equalize(void *h, int stream, const mskf_fe_equalize *cfg) {
    if (!cfg) return MSKF_ERR_INVALID;
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setEqualize(*cfg); });
}
// ImageProcessor::setInputFormat (mskf_fe_set_input_format) of one stream, or of all (stream < 0); call before the first frame.
// The images of mskfh_runner_step and the frames of mskfh_runner_set_sequence are then raw byte rasters in that format.
// All or nothing: a stream that refuses (bad arguments refuse at the first stream; a pending batch or a failed allocation may refuse
// at a later one) ends the call with its status, and the streams switched before it get their previous setting back.
int mskfh_runner_set_input_format(void *h, int stream, const mskf_fe_input_format *cfg) {
    MultiRunner *r = (MultiRunner *)h;
    if (!cfg || stream >= r->n_streams()) return MSKF_ERR_INVALID;
    std::vector<mskf_fe_input_format> before;
    for (int i = 0; i < r->n_streams(); ++i) before.push_back(r->system(i).imgproc_ptr_->inputFormat());
    for (int i = 0; i < r->n_streams(); ++i) {
        if (stream >= 0 && i != stream) continue;
        const int rc = r->system(i).imgproc_ptr_->setInputFormat(*cfg);
        if (rc == MSKF_OK) continue;
        for (int k = 0; k < i; ++k)
            if (stream < 0 || k == stream) (void)r->system(k).imgproc_ptr_->setInputFormat(before[k]);      // (a success leaves mskf_last_error as it is)
        return rc;
    }
    return MSKF_OK;
}
// ImageProcessor::setMask (mskf_fe_set_mask) of one stream, or of all (stream < 0); between runs.  Returns the first status that
// is not MSKF_OK (mskf_last_error has the text): bad arguments refuse at the first stream, which then keeps its previous masks.
int mskfh_runner_set_mask(void *h, int stream, const mskf_fe_mask *cfg) {
    if (!cfg) return MSKF_ERR_INVALID;
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setMask(cfg->cam0, cfg->cam1, cfg->width, cfg->height, cfg->pitch, cfg->margin); });
}
// ImageProcessor::setPatchCheck (mskf_fe_set_patch_check) of one stream, or of all (stream < 0); between runs.  Returns the first
// status that is not MSKF_OK (mskf_last_error has the text): bad arguments refuse at the first stream, which keeps its setting.
int mskfh_runner_set_patch_check(void *h, int stream, const mskf_fe_patch_check *cfg) {
    if (!cfg) return MSKF_ERR_INVALID;
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setPatchCheck(*cfg); });
}
// the optional patch_check keys of an app_imgproc.yaml (patch_check_from_yaml); 0 on success
int mskfh_load_patch_check(const char *yaml_path, mskf_fe_patch_check *out) {
    try {
        *out = patch_check_from_yaml(YAML::LoadFile(yaml_path));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mskfh_load_patch_check: %s\n", e.what());
        return -1;
    }
}
// ImageProcessor::setFbCheck (mskf_fe_set_fb_check) of one stream, or of all (stream < 0); between runs.  As mskfh_runner_set_patch_check.
int mskfh_runner_set_fb_check(void *h, int stream, const mskf_fe_fb_check *cfg) {
    if (!cfg) return MSKF_ERR_INVALID;
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setFbCheck(*cfg); });
}
// the optional fb_check keys of an app_imgproc.yaml (fb_check_from_yaml); 0 on success
int mskfh_load_fb_check(const char *yaml_path, mskf_fe_fb_check *out) {
    try {
        *out = fb_check_from_yaml(YAML::LoadFile(yaml_path));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mskfh_load_fb_check: %s\n", e.what());
        return -1;
    }
}
// ImageProcessor::setLkLevels (mskf_fe_set_lk_levels) of one stream, or of all (stream < 0); before the streams' first frame.
int mskfh_runner_set_lk_levels(void *h, int stream, int levels) {
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setLkLevels(levels); });
}
// the optional lk_pyramid_levels key of an app_imgproc.yaml, for a width x height image (lk_levels_from_yaml); 0 on success, and the
// reason of a refusal is kept, per thread, for mskfh_load_lk_levels_error
static thread_local std::string g_lk_levels_error;      // (per thread: loaders may run side by side)
int mskfh_load_lk_levels(const char *yaml_path, int width, int height, int *out) {
    try {
        *out = lk_levels_from_yaml(YAML::LoadFile(yaml_path), width, height);
        return 0;
    } catch (const std::exception &e) {
        g_lk_levels_error = e.what();
        std::fprintf(stderr, "mskfh_load_lk_levels: %s\n", e.what());
        return -1;
    }
}
const char *mskfh_load_lk_levels_error(void) { return g_lk_levels_error.c_str(); }
// ImageProcessor::setCameraModel (mskf_fe_set_camera_model) of one stream, or of all (stream < 0); between runs.  As mskfh_runner_set_fb_check.
int mskfh_runner_set_camera_model(void *h, int stream, const mskf_fe_camera_model *cfg) {
    if (!cfg) return MSKF_ERR_INVALID;
    return set_on_streams(h, stream, [&](ImageProcessor &ip) { return ip.setCameraModel(*cfg); });
}
// the camera models of a camchain yaml (camera_models_from_yaml): out[2], extended[2]; 0 on success
int mskfh_load_camera_models(const char *yaml_path, mskf_fe_camera_model *out, int *extended) {
    try {
        const YAML::Node n = YAML::LoadFile(yaml_path);
        (void)calib_from_yaml(n);
        const CamchainModels m = camera_models_from_yaml(n);
        for (int c = 0; c < 2; ++c) { out[c] = m.cam[c]; extended[c] = m.extended[c] ? 1 : 0; }
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mskfh_load_camera_models: %s\n", e.what());
        return -1;
    }
}
// ImageProcessor::setDescriptors of one stream, or of all (stream < 0); between runs, from the next frame on
int mskfh_runner_set_descriptors(void *h, int stream, int on) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream >= r->n_streams()) return MSKF_ERR_INVALID;
    for (int i = 0; i < r->n_streams(); ++i) if (stream < 0 || i == stream) r->system(i).imgproc_ptr_->setDescriptors(on != 0);
    return MSKF_OK;
}
// the descriptors of the stream's last frame, aligned with its message: ids, 32 bytes each, validity; 0 entries with the option off
int mskfh_num_descriptors(void *h, int stream) { return (int)((MultiRunner *)h)->system(stream).imgproc_ptr_->descriptorIds().size(); }
void mskfh_get_descriptors(void *h, int stream, uint64_t *ids, uint8_t *desc, uint8_t *valid) {
    const ImageProcessor &ip = *((MultiRunner *)h)->system(stream).imgproc_ptr_;
    const size_t n = ip.descriptorIds().size();
    for (size_t i = 0; i < n; ++i) ids[i] = ip.descriptorIds()[i];
    if (n) { std::memcpy(desc, ip.descriptors().data(), 32 * n); std::memcpy(valid, ip.descriptorValid().data(), n); }
}
// ---- keyframes (keyframes.h): stored copies of a stream's last-frame descriptors and their matching; between runs.
// The stream's last frame (time, ids, desc, valid) becomes a keyframe; returns its index, -1 with descriptors off for the stream.
int mskfh_add_keyframe(void *h, int stream) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream < 0 || stream >= r->n_streams()) return -1;
    ImageProcessor &ip = *r->system(stream).imgproc_ptr_;
    if (!ip.descriptorsOn()) return -1;
    return ip.keyframes.add(ip.descriptorTime(), std::vector<uint64_t>(ip.descriptorIds().begin(), ip.descriptorIds().end()), ip.descriptors(), ip.descriptorValid(), ip.descriptorObs());
}
int mskfh_num_keyframes(void *h, int stream) { return ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.size(); }
// the feature count of keyframe k, -1: no such keyframe
int mskfh_keyframe_size(void *h, int stream, int k) {
    const KeyframeStore &s = ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes;
    return k < 0 || k >= s.size() ? -1 : (int)s.at(k).ids.size();
}
void mskfh_get_keyframe(void *h, int stream, int k, double *time, uint64_t *ids, uint8_t *desc, uint8_t *valid) {
    const Keyframe &f = ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.at(k);
    *time = f.time;
    const size_t n = f.ids.size();
    if (n) { std::memcpy(ids, f.ids.data(), 8 * n); std::memcpy(desc, f.desc.data(), 32 * n); std::memcpy(valid, f.valid.data(), n); }
}
void mskfh_clear_keyframes(void *h, int stream) {      // of one stream, or of all (stream < 0)
    MultiRunner *r = (MultiRunner *)h;
    for (int i = 0; i < r->n_streams(); ++i) if (stream < 0 || i == stream) r->system(i).imgproc_ptr_->keyframes.clear();
}
// The stream's last-frame descriptors against every keyframe of the stream, one mskf_fe_match_batch on the stream's context.
// Returns the number of keyframes with n_matches >= min_matches (mskfh_keyframe_hit reads them), or a negative mskf status.
int mskfh_query_keyframes(void *h, int stream, int max_distance, float ratio, int cross_check, int min_matches) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream < 0 || stream >= r->n_streams()) return MSKF_ERR_INVALID;
    ImageProcessor &ip = *r->system(stream).imgproc_ptr_;
    if (!ip.descriptorsOn()) { return MSKF_ERR_INVALID; }
    int local;
    const int rc = ip.keyframes.query(r->group_of(stream, local).ctx(), ip.descriptorTime(), std::vector<uint64_t>(ip.descriptorIds().begin(), ip.descriptorIds().end()), ip.descriptors(),
                                      ip.descriptorValid(), max_distance, ratio, cross_check != 0, min_matches);
    return rc != MSKF_OK ? rc : (int)ip.keyframes.hits().size();
}
// hit i of the last query: the keyframe's index, time and match count; pairs (when not null) takes 2 * n_matches ids
void mskfh_keyframe_hit(void *h, int stream, int i, int *k, double *time, int *n_matches, uint64_t *pairs) {
    const KeyframeHit &hit = ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.hits()[i];
    *k = hit.k; *time = hit.time; *n_matches = hit.n_matches;
    if (pairs && !hit.pairs.empty()) std::memcpy(pairs, hit.pairs.data(), 8 * hit.pairs.size());
}
// the stereo observations of keyframe k: 4 doubles per feature (mskfh_keyframe_size of them)
void mskfh_get_keyframe_obs(void *h, int stream, int k, double *obs) {
    const Keyframe &f = ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.at(k);
    if (!f.obs.empty()) std::memcpy(obs, f.obs.data(), 8 * f.obs.size());
}
// The stereo RANSAC pose check of every hit of the stream's last mskfh_query_keyframes against the stream's last frame, one
// mskf_fe_verify_batch on the stream's context.  Returns the number of records (one per hit; mskfh_keyframe_verification reads
// them), or a negative mskf status (stale hits among them: mskf_last_error names the reason).
int mskfh_verify_keyframes(void *h, int stream, int n_hypotheses, uint64_t seed, double max_error, double min_depth, double max_depth) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream < 0 || stream >= r->n_streams()) return MSKF_ERR_INVALID;
    ImageProcessor &ip = *r->system(stream).imgproc_ptr_;
    if (!ip.descriptorsOn()) return MSKF_ERR_INVALID;
    int local;
    std::string why;
    const int rc = ip.keyframes.verify(r->group_of(stream, local).ctx(), ip.descriptorTime(), std::vector<uint64_t>(ip.descriptorIds().begin(), ip.descriptorIds().end()),
                                       ip.descriptorObs(), ip.stereoExtrinsics(), n_hypotheses, seed, max_error, min_depth, max_depth, why);
    ip.keyframes.refused = why;               // empty: the status is mskf_fe_verify_batch's own, and mskf_last_error has its reason
    return rc != MSKF_OK ? rc : (int)ip.keyframes.verified().size();
}
// why the store itself refused the last mskfh_verify_keyframes of the stream ("" when it did not)
const char *mskfh_verify_refused(void *h, int stream) { return ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.refused.c_str(); }
// record i of the last verification: ints = k, n_matches, n_usable, n_inliers, best, status; doubles = time, rms, R[9], t[3],
// info[36] (50 of them); inlier (when not null) takes n_matches bytes, one per pair of the hit
void mskfh_keyframe_verification(void *h, int stream, int i, int *ints, double *doubles, uint8_t *inlier) {
    const KeyframeVerification &v = ((MultiRunner *)h)->system(stream).imgproc_ptr_->keyframes.verified()[i];
    ints[0] = v.k; ints[1] = v.n_matches; ints[2] = v.n_usable; ints[3] = v.n_inliers; ints[4] = v.best; ints[5] = v.status;
    doubles[0] = v.time; doubles[1] = v.rms;
    std::memcpy(doubles + 2, v.R, sizeof(v.R)); std::memcpy(doubles + 11, v.t, sizeof(v.t)); std::memcpy(doubles + 14, v.info, sizeof(v.info));
    if (inlier && !v.inlier.empty()) std::memcpy(inlier, v.inlier.data(), v.inlier.size());
}
// MsckfVio::publishCovariance of one stream, or of all (stream < 0); set before the first frame
void mskfh_runner_publish_covariance(void *h, int stream, int on) {
    MultiRunner *r = (MultiRunner *)h;
    for (int i = 0; i < r->n_streams(); ++i) if (stream < 0 || i == stream) r->system(i).msckfvio_ptr()->publishCovariance = on != 0;
}
// MsckfVio::setZupt of one stream, or of all (stream < 0); between runs
int mskfh_runner_set_zupt(void *h, int stream, int on, double max_disparity, int min_features, double noise_std) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream >= r->n_streams() || !(max_disparity > 0) || !(noise_std > 0) || min_features < 0 || max_disparity > 1e300 || noise_std > 1e300) return MSKF_ERR_INVALID;
    zupt::Config c;
    c.on = on != 0; c.max_disparity = max_disparity; c.min_features = min_features; c.noise_std = noise_std;
    for (int i = 0; i < r->n_streams(); ++i) if (stream < 0 || i == stream) r->system(i).msckfvio_ptr()->setZupt(c);
    return MSKF_OK;
}
// MsckfVio::queueVelocity (kind 0) / queuePosition (kind 1) of one stream; between runs
int mskfh_runner_fuse(void *h, int stream, int kind, double t, const double *z, const double *R, int gated) {
    MultiRunner *r = (MultiRunner *)h;
    if (stream < 0 || stream >= r->n_streams() || !z || !R || (kind != 0 && kind != 1)) return MSKF_ERR_INVALID;
    MsckfVio &v = *r->system(stream).msckfvio_ptr();
    return (kind == 0 ? v.queueVelocity(t, z, R, gated != 0) : v.queuePosition(t, z, R, gated != 0)) ? MSKF_OK : MSKF_ERR_INVALID;
}
int mskfh_num_direct_updates(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numDirectUpdates(); }
int mskfh_num_zupt(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numZupt(); }
int mskfh_num_odom_covs(void *h, int stream) { return (int)((MultiRunner *)h)->system(stream).msckfvio_ptr()->odomCovs().size(); }
void mskfh_get_odom_covs(void *h, int stream, mskf_odom_cov *out) {
    const auto &c = ((MultiRunner *)h)->system(stream).msckfvio_ptr()->odomCovs();
    std::memcpy(out, c.data(), c.size() * sizeof(mskf_odom_cov));
}
int mskfh_state_dim(void *h, int stream) { int d = 0; mskf_ekf_get_dim(((MultiRunner *)h)->system(stream).stream(), &d); return d; }
int mskfh_get_cov(void *h, int stream, double *out, int cap) { return mskf_ekf_get_cov(((MultiRunner *)h)->system(stream).stream(), out, cap); }
void mskfh_get_imu_state(void *h, int stream, double *out) {   // same 28-double layout as the oracle's getter
    const IMUState &s = ((MultiRunner *)h)->system(stream).msckfvio_ptr()->imuState();
    int k = 0;
    for (int i = 0; i < 4; ++i) out[k++] = s.orientation.q[i];
    for (int i = 0; i < 3; ++i) out[k++] = s.position[i];
    for (int i = 0; i < 3; ++i) out[k++] = s.velocity[i];
    for (int i = 0; i < 3; ++i) out[k++] = s.gyro_bias[i];
    for (int i = 0; i < 3; ++i) out[k++] = s.acc_bias[i];
    for (int i = 0; i < 9; ++i) out[k++] = s.R_imu_cam0.m[i];
    for (int i = 0; i < 3; ++i) out[k++] = s.t_cam0_imu[i];
}
long long mskfh_num_device_frames(void *h, int stream) { return ((MultiRunner *)h)->system(stream).imgproc_ptr_->deviceFrames(); }
int mskfh_num_updates(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numUpdates(); }
int mskfh_num_tsqr_updates(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numTsqrUpdates(); }
int mskfh_num_uncompressed_updates(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numUncompressedUpdates(); }
long long mskfh_stacked_rows(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->stackedRows(); }
long long mskfh_num_resets(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numResets(); }
int mskfh_num_clones(void *h, int stream) { return ((MultiRunner *)h)->system(stream).msckfvio_ptr()->numClones(); }
void *mskfh_group_hip_stream(void *h, int stream) { int l; return mskf_ctx_hip_stream(((MultiRunner *)h)->group_of(stream, l).ctx()); }

}  // extern "C"
