// system.h — host mirror of cg::System (reference msckf_core/include/system.h:16-41, src/system.cpp:11-54):
// one ImageProcessor + one MsckfVio sharing one device stream, three relay callbacks.
#pragma once
#include <string>
#include "image_processor.h"
#include "msckf_vio.h"

namespace cg {

class System {
  public:
    // reference constructor: camchain YAML path, app_*.yaml read from ../config (Q16); GPU 0
    explicit System(std::string file_cam_imu);
    // explicit configuration; ctx == nullptr creates a private context on `device`
    System(const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf, mskf_ctx *ctx = nullptr, int device = 0);
    ~System();

    void stereo_callback(const cg::Image &cam0_img, const cg::Image &cam1_img, bool is_draw = false);
    void imu_callback(const cg::ImuConstPtr &msg);
    void backend_callback();

    std::vector<cg::Vector3> path_to_draw_;
    std::vector<cg::Point3f> points3d_to_draw_;
    cg::ImageProcessorPtr imgproc_ptr_;

    typedef std::shared_ptr<System> Ptr;
    typedef std::shared_ptr<const System> ConstPtr;

    // access for BatchRunner / tests
    cg::MsckfVioPtr msckfvio_ptr() const { return msckfvio_ptr_; }
    std::shared_ptr<CameraMeasurement> feature_msg() const { return feature_msg_ptr_; }
    void set_feature_msg(const std::shared_ptr<CameraMeasurement> &m) { feature_msg_ptr_ = m; }
    mskf_stream *stream() const { return stream_; }
    bool ok() const { return ok_; }
    // the mask files app_imgproc.yaml names (mask_files_from_yaml; the YAML constructor reads them): the application loads them
    // with its image reader and calls imgproc_ptr_->setMask before the first frame
    const MaskFiles &maskFiles() const { return mask_files_; }
    bool copy_draw_buffers = true;   // backend_callback copies path_/points3d_ every frame in the reference (Q20)

  private:
    void setup(const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf, mskf_ctx *ctx, int device);
    YAML::Node cfg_cam_imu_;
    mskf_fe_input_format input_format_{0, 0};          // likewise (input_format_from_yaml)
    mskf_fe_equalize equalize_{0, 8, 8, 0, 40.0};      // the YAML constructor reads it from app_imgproc.yaml (equalize_from_yaml)
    MaskFiles mask_files_;
    mskf_fe_patch_check patch_check_{0, 4, 0.8f, 0.8f};  // likewise (patch_check_from_yaml)
    mskf_fe_fb_check fb_check_{0, 1.0f, 1.0f};          // likewise (fb_check_from_yaml)
    int lk_levels_ = 4;                                 // likewise (lk_levels_from_yaml)
    CamchainModels camera_models_{{}, {false, false}};  // the camchain's extended camera models (camera_models_from_yaml); none by default
    bool descriptors_ = false;                         // likewise (descriptors_from_yaml)
    std::shared_ptr<CameraMeasurement> feature_msg_ptr_;
    cg::MsckfVioPtr msckfvio_ptr_;
    mskf_ctx *own_ctx_ = nullptr;
    mskf_stream *stream_ = nullptr;
    bool ok_ = false;
};

typedef System::Ptr SystemPtr;
typedef System::ConstPtr SystemConstPtr;

}  // namespace cg
