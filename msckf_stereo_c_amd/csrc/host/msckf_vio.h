// msckf_vio.h — host mirror of cg::MsckfVio (reference msckf_core/include/msckf_vio.h:35-200) with the
// state structs of common/imu_state.h, common/cam_state.h and the Feature bookkeeping of feature.hpp.
//
// Same public surface (ctor from the camchain YAML node, initialize(), resetCallback(), imuCallback(),
// featureCallback(), get_path(), get_points3d()).  The covariance never leaves the GPU: propagation,
// augmentation, triangulation, Jacobians, gating, QR and the Kalman update run behind the C-ABI
// (include/mskf_hip.h); this class integrates the 16-dim nominal state, keeps the clone / feature maps
// and applies the returned correction vector.  The order of a frame (phaseA -> predict -> update -> phaseB -> update ->
// phaseC -> clone removal -> [direct updates of the streams that have one due -> correction -> publish] -> read-out -> phaseD) is written once, over n streams, in runFrame(): featureCallback() is
// runFrame() with n = 1, BatchGroup calls it with its group.  The phases themselves never touch the device.
#pragma once
#include <array>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../../include/mskf_hip.h"
#include "cg_types.h"
#include "feature_store.h"
#include "frame_seq.h"
#include "yaml_lite.h"
#include "zupt.h"

namespace cg {

mskf_ekf_cfg ekf_cfg_from_yaml(const YAML::Node &cfg_msckfvio);
// optional keys of app_msckfvio.yaml (not keys of the reference's file): zupt: on | off, zupt_max_disparity, zupt_min_features,
// zupt_noise_std; absent means off (zupt.h)
zupt::Config zupt_cfg_from_yaml(const YAML::Node &cfg_msckfvio);

struct Quat { double q[4] = {0, 0, 0, 1}; };   // JPL [x y z w]

struct IMUState {   // common/imu_state.h:28-88; the class statics live in MsckfVio (per stream)
    StateIDType id = 0;
    double time = 0;
    Quat orientation;
    Vector3 position, velocity, gyro_bias, acc_bias;
    hm::Mat3 R_imu_cam0 = hm::Mat3::identity();
    Vector3 t_cam0_imu;
    Quat orientation_null;
    Vector3 position_null, velocity_null;
};

struct CAMState {   // common/cam_state.h:25-55
    StateIDType id = 0;
    double time = 0;
    Quat orientation;
    Vector3 position;
    Quat orientation_null;
    Vector3 position_null;
    int slot = -1;      // row of the observation table that holds this clone's observations (feature_store.h)
};
typedef std::map<StateIDType, CAMState> CamStateServer;
// Feature / MapServer (feature.hpp:31-168): see feature_store.h — flat tables with the maps' semantics

class MsckfVio {
  public:
    explicit MsckfVio(YAML::Node cfg_cam_imu);
    MsckfVio(const mskf_calib &calib, const mskf_ekf_cfg &cfg);
    MsckfVio(const MsckfVio &) = delete;
    MsckfVio operator=(const MsckfVio &) = delete;
    ~MsckfVio();

    bool initialize();
    bool resetCallback();
    void imuCallback(const cg::ImuConstPtr &msg);
    void featureCallback(const CameraMeasurementConstPtr &msg);
    std::vector<cg::Vector3> get_path() { return path_; }
    std::vector<cg::Point3f> get_points3d() { return points3d_; }

    typedef std::shared_ptr<MsckfVio> Ptr;
    typedef std::shared_ptr<const MsckfVio> ConstPtr;

    // ---- the filter of one frame of n streams of one (filter) context: phaseA -> mskf_ekf_predict_batch (IMU propagation +
    // augmentation) -> lost-feature update batch -> phaseB -> pruning update batch -> phaseC -> mskf_ekf_remove_clones_batch ->
    // odometry covariances (publishCovariance on any stream), or the position variances on their own when an active stream
    // needs them (position_std_threshold > 0) and no update of the frame brought them back -> phaseD.  The update batches take
    // the streams with features only.  `par`, `acc`, the return value and `err`: as ImageProcessor::runFrame.
    struct FrameScratch {      // argument records of the frame's calls
        std::vector<mskf_ekf_update_args> u, upd_a;           // per stream; of the streams with a non-empty update (with upd_s: valid until *_end)
        std::vector<mskf_stream *> upd_s;
        std::vector<int32_t> pred_ns, rm;                     // prediction steps and clone removals per stream
        std::vector<const mskf_imu_step *> pred_sp; std::vector<const double *> pred_jp;
        std::vector<double> pv; std::vector<mskf_odom_cov> oc;   // position variances fetched on their own (3 per stream); odometry covariances
        std::vector<mskf_ekf_direct_args> dir_a; std::vector<mskf_stream *> dir_s; std::vector<int> dir_i;   // the streams with a direct update due (valid until *_end)
    };
    static int runFrame(mskf_ctx *ekf_ctx, int n, MsckfVio *const *vio, mskf_stream *const *streams, const CameraMeasurementConstPtr *msgs,
                        FrameScratch &scratch, const ParFor &par, double *acc, std::string &err);

    // ---- device attachment + the phases runFrame() runs (host only: what the device is to do they leave in predictSteps() /
    // predictJ(), the update arguments and pendingRemovals())
    void attach(mskf_stream *s) { stream_ = s; }
    mskf_stream *stream() const { return stream_; }
    // phase A: IMU propagation and augmentation of the nominal state, observations; fills the lost-feature update (n_feat may be 0)
    bool phaseA(const CameraMeasurementConstPtr &msg, mskf_ekf_update_args &upd);
    const std::vector<mskf_imu_step> &predictSteps() const { return imu_steps_; }
    const double *predictJ() const { return have_J_ ? J_ : nullptr; }
    // phase B: apply the lost-feature update, then prepare the pruning update (n_feat may be 0)
    void phaseB(mskf_ekf_update_args &upd);
    // phase C: apply the pruning update, delete clones (the device's copies: pendingRemovals()), publish
    void phaseC();
    const int32_t *pendingRemovals() const { return pending_rm_; }   // two clone indices (current state order) or -1
    // ---- opt-in direct measurements (mskf_ekf_update_direct*): world-frame measurements z of the IMU's velocity (error states 6..8)
    // or position (12..14) with covariance R (3 x 3 row-major, symmetric, positive diagonal), applied in the first filter frame whose
    // time stamp is >= t: r = z - state, H the selector, gated at the 95 % chi-square value of 3 degrees of freedom when `gated`.
    // A frame applies everything that is due, oldest first, one update batch per round, behind the clone removal; the published
    // pose of such a frame carries the corrections (publish moves from phaseC behind them).  false: R refused, nothing queued.
    // resetCallback and an online reset (phaseD) empty the queue: what was measured against the old state is not applied to the new.
    bool queueVelocity(double t, const double z[3], const double R[9], bool gated) { return queueDirect(6, t, z, R, gated, false); }
    bool queuePosition(double t, const double z[3], const double R[9], bool gated) { return queueDirect(12, t, z, R, gated, false); }
    // zero-velocity update: with c.on every frame compares the cam0 points of its message with the previous message's (zupt.h) and a
    // stationary pair queues z = 0 on the velocity with R = noise_std^2 I, gated
    void setZupt(const zupt::Config &c) { zupt_ = c; zupt_prev_.clear(); zupt_have_prev_ = false; }
    const zupt::Config &zuptConfig() const { return zupt_; }
    bool directDue() const;                                  // a queued measurement applies in this frame
    void buildDirect(mskf_ekf_direct_args &a);               // the oldest due measurement, against the state as it is now
    void finishDirect(const mskf_ekf_direct_args &a);        // its correction, counters, position variances
    void publishDeferred();                                  // the publish a frame with a direct update postponed in phaseC
    int numDirectUpdates() const { return n_direct_updates_; }   // direct updates applied (status 1), zero-velocity updates included
    int numZupt() const { return n_zupt_; }                      // ... of which zero-velocity updates
    // phase D: online reset decision from the position variances (msckf_vio.cpp:1186-1236)
    void phaseD(const double pos_var[3]);
    // the position variances the last update of this frame brought back (mskf_ekf_update_args.pos_var_out), if any
    bool havePosVar() const { return pos_var_valid_; }
    const double *posVar() const { return pos_var_; }
    bool frameActive() const { return frame_active_; }
    void enableFileOutputs() {   // msckf_vio.cpp:169-171
        if (!pose_outfile_.is_open()) pose_outfile_.open("pose_out.txt");
        if (!debug_.is_open()) debug_.open("debug_msckfvio.txt");
    }
    // optional: records [start, size) of `msg` are untouched value-initialised records (Q1 tail)
    // total_size > msg->features.size(): `msg` is a snapshot truncated inside the zero tail of a longer message
    void setZeroTailHint(const CameraMeasurement *msg, size_t start, size_t total_size = 0) {
        zero_tail_msg_ = msg; zero_tail_start_ = start; zero_tail_total_ = total_size;
    }

    const std::vector<mskf_pose> &poses() const { return poses_; }
    // publishCovariance: one record per pose, indexed like poses() (empty while the switch has never been on)
    const std::vector<mskf_odom_cov> &odomCovs() const { return odom_covs_; }
    // the covariance half of publish() (msckf_vio.cpp:1262-1293) for the pose just published; the caller read it with
    // mskf_ekf_get_odom_cov* after the frame's updates and clone removal, before onlineReset (phaseD)
    void attachOdomCov(const mskf_odom_cov &c);
    void enableCovarianceOutput(const std::string &path) {   // one line per pose: time stamp, 36 pose entries, 9 twist entries
        publishCovariance = true;
        if (!cov_outfile_.is_open()) cov_outfile_.open(path);
    }
    const IMUState &imuState() const { return state_server.imu_state; }
    int numClones() const { return (int)state_server.cam_states.size(); }
    int numUpdates() const { return n_update_; }
    // diagnostics of the QR compression (include/mskf_hip.h diag_out): updates that ran as Householder TSQR, sum of stacked rows
    int numTsqrUpdates() const { return n_tsqr_; }
    int numUncompressedUpdates() const { return n_direct_; }
    long long stackedRows() const { return rows_sum_; }
    long long numResets() const { return online_reset_counter_; }
    size_t mapSize() const { return map_server.size(); }
    bool keepTrajectory = true;   // path_/points3d_ grow forever in the reference (Q20); benches may switch it off
    bool publishCovariance = false;   // publish()'s pose / velocity covariance (:1262-1293), read from the device once per frame; set before the first frame
    const std::string &error() const { return error_; }

  private:
    struct StateServer {
        IMUState imu_state;
        CamStateServer cam_states;
    } state_server;

    bool loadParameters();
    void resetCov();
    void initializeGravityAndBias();
    void batchImuProcessing(double time_bound);
    void predictNewState(double dt, const Vector3 &gyro, const Vector3 &acc);
    void stateAugmentation(double time);
    void addFeatureObservations(const CameraMeasurementConstPtr &msg);
    void buildLostFeatureUpdate(mskf_ekf_update_args &upd);
    void findRedundantCamStates(std::vector<StateIDType> &rm);
    void buildPruneUpdate(mskf_ekf_update_args &upd);
    void applyCorrection(const std::vector<double> &delta_x);
    void applyStateCorrection(const std::vector<double> &delta_x);   // the state part alone (a direct update counts as no feature update)
    bool queueDirect(int first_col, double t, const double z[3], const double R[9], bool gated, bool is_zupt);
    void zuptObserve(const CameraMeasurementConstPtr &msg);
    void publish(double time_stamp);
    bool checkMotion(int slot, uint64_t mask) const;
    void packClones();
    int allocCloneSlot();
    void resetCloneSlots();
    void finishArgs(mskf_ekf_update_args &upd, int dof_offset, int apply_cap);
    void fail(const char *what, int rc);
    void dumpFeatureJacobians();   // debug_msckfvio.txt, frame n_pub == 9 (msckf_vio.cpp:719-723)

    YAML::Node cfg_cam_imu_;
    bool have_yaml_ = false;
    mskf_calib calib_;
    mskf_ekf_cfg cfg_;
    mskf_stream *stream_ = nullptr;
    std::string error_;

    // the reference's class statics (msckf_vio.cpp:33-47), per stream here
    StateIDType next_state_id_ = 0;
    double gyro_noise_ = 0, acc_noise_ = 0, gyro_bias_noise_ = 0, acc_bias_noise_ = 0, observation_noise_ = 0;
    Vector3 gravity_{0, 0, -9.81};
    hm::Rigid T_imu_body_, T_cam0_cam1_;
    double feat_translation_threshold_ = 0.2;

    std::vector<cg::Vector3> path_;
    std::vector<cg::Point3f> points3d_;
    std::vector<mskf_pose> poses_;
    std::vector<mskf_odom_cov> odom_covs_;
    MapServer map_server;
    std::vector<cg::Imu> imu_msg_buffer;
    bool is_gravity_set = false;
    bool is_first_img = true;
    double tracking_rate = 0;
    int n_update_ = 0;
    long long online_reset_counter_ = 0;
    bool frame_active_ = false;
    double frame_time_ = 0;

    // per-frame staging shared between phases
    std::vector<mskf_imu_step> imu_steps_;
    std::vector<mskf_clone_state> clones_;
    std::vector<mskf_ekf_feature> feats_;
    std::vector<int> feat_slots_;                          // map_server slots of feats_
    std::vector<size_t> erase_ranks_;                      // map_server ranks to erase after the lost-feature update (ascending)
    std::vector<int> order_slot_;                          // observation-table row of the k-th oldest clone (packClones)
    std::vector<int> free_clone_slots_;
    std::vector<int32_t> obs_clone_;
    std::vector<double> obs_z_;
    std::vector<double> delta_x_, gamma_;
    std::vector<uint8_t> feat_status_;
    int32_t rows_out_ = 0;
    int32_t diag_out_[2] = {0, 0};
    double pos_var_[3] = {-1, -1, -1}, pos_var_buf_[3] = {-1, -1, -1};
    bool pos_var_valid_ = false;
    void takePosVar() { if (pos_var_buf_[0] >= 0) { pos_var_[0] = pos_var_buf_[0]; pos_var_[1] = pos_var_buf_[1]; pos_var_[2] = pos_var_buf_[2]; pos_var_valid_ = true; } }
    int n_tsqr_ = 0, n_direct_ = 0;
    long long rows_sum_ = 0;
    std::vector<StateIDType> rm_cam_state_ids_;
    bool prune_pending_ = false;
    bool have_J_ = false;
    double J_[6 * 21];
    int32_t pending_rm_[2] = {-1, -1};
    int rm_order_[2] = {-1, -1};                           // window positions of the two clones being pruned
    // direct measurements: the queue (insertion order), the one in flight and its argument arrays
    struct DirectMeas { int first_col; double t, z[3], R[9]; bool gated, is_zupt; };
    std::vector<DirectMeas> direct_queue_;
    DirectMeas direct_cur_{};
    double dH_[3 * 21], dr_[3];
    std::vector<double> ddx_;
    int n_direct_updates_ = 0, n_zupt_ = 0;
    bool publish_deferred_ = false;
    zupt::Config zupt_;
    std::vector<zupt::Point> zupt_prev_, zupt_curr_;
    zupt::Scratch zupt_scratch_;
    bool zupt_have_prev_ = false;
    const CameraMeasurement *zero_tail_msg_ = nullptr;
    size_t zero_tail_start_ = 0, zero_tail_total_ = 0;
    std::ofstream pose_outfile_, debug_, cov_outfile_;
    int n_pub_ = 0;                                        // published frames (msckf_vio.cpp:356)
};

typedef MsckfVio::Ptr MsckfVioPtr;
typedef MsckfVio::ConstPtr MsckfVioConstPtr;

}  // namespace cg
