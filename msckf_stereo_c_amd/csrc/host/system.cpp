// system.cpp — see system.h.  Reference: msckf_core/src/system.cpp:11-54.
#include "system.h"
#include <iostream>

namespace cg {

System::System(std::string file_cam_imu) : feature_msg_ptr_(new CameraMeasurement) {
    try {
        cfg_cam_imu_ = YAML::LoadFile(file_cam_imu);
        mskf_calib calib = calib_from_yaml(cfg_cam_imu_);
        camera_models_ = camera_models_from_yaml(cfg_cam_imu_);
        const YAML::Node cfg_imgproc = YAML::LoadFile("../config/app_imgproc.yaml");
        mskf_fe_cfg fe = fe_cfg_from_yaml(cfg_imgproc);
        equalize_ = equalize_from_yaml(cfg_imgproc);
        input_format_ = input_format_from_yaml(cfg_imgproc);
        mask_files_ = mask_files_from_yaml(cfg_imgproc);
        patch_check_ = patch_check_from_yaml(cfg_imgproc);
        fb_check_ = fb_check_from_yaml(cfg_imgproc);
        lk_levels_ = lk_levels_from_yaml(cfg_imgproc, calib.width, calib.height);
        descriptors_ = descriptors_from_yaml(cfg_imgproc);
        const YAML::Node cfg_msckfvio = YAML::LoadFile("../config/app_msckfvio.yaml");
        mskf_ekf_cfg ekf = ekf_cfg_from_yaml(cfg_msckfvio);
        setup(calib, fe, ekf, nullptr, 0);
        if (ok_) { imgproc_ptr_->enableFileOutputs(); msckfvio_ptr_->enableFileOutputs(); }   // pose_out.txt, debug_imageprocessor.txt
        // optional (not a key of the reference's file): "descriptors_out: <file>" writes the published features' descriptors
        if (ok_ && cfg_imgproc["descriptors_out"].IsDefined()) imgproc_ptr_->enableDescriptorOutput(cfg_imgproc["descriptors_out"].as<std::string>());
        if (ok_) msckfvio_ptr_->setZupt(zupt_cfg_from_yaml(cfg_msckfvio));        // optional keys zupt*: absent means off
        // optional (not a key of the reference's file): "covariance_out: <file>" writes publish()'s covariances, one line per pose
        if (ok_ && cfg_msckfvio["covariance_out"].IsDefined()) msckfvio_ptr_->enableCovarianceOutput(cfg_msckfvio["covariance_out"].as<std::string>());
    } catch (const std::exception &e) {   // the reference swallows init errors and only prints (system.cpp:17-33)
        std::cerr << "Cannot initialize System: " << e.what() << std::endl;
    }
}

System::System(const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf, mskf_ctx *ctx, int device)
    : feature_msg_ptr_(new CameraMeasurement) {
    setup(calib, fe, ekf, ctx, device);
}

void System::setup(const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf, mskf_ctx *ctx, int device) {
    if (!ctx) {
        int rc = mskf_ctx_create(device, &own_ctx_);
        if (rc != MSKF_OK) { std::cerr << "Cannot create the device context: " << mskf_last_error() << std::endl; return; }
        ctx = own_ctx_;
    }
    int rc = mskf_stream_create(ctx, &calib, &fe, &ekf, &stream_);
    if (rc != MSKF_OK) { std::cerr << "Cannot create the device stream: " << mskf_last_error() << std::endl; return; }
    imgproc_ptr_.reset(new cg::ImageProcessor(calib, fe));
    imgproc_ptr_->attach(stream_);
    imgproc_ptr_->setEqualize(equalize_);      // (kept until initialize())
    imgproc_ptr_->setInputFormat(input_format_);
    imgproc_ptr_->setPatchCheck(patch_check_);
    imgproc_ptr_->setFbCheck(fb_check_);
    imgproc_ptr_->setLkLevels(lk_levels_);
    for (int c = 0; c < 2; ++c) if (camera_models_.extended[c]) imgproc_ptr_->setCameraModel(camera_models_.cam[c]);
    imgproc_ptr_->setDescriptors(descriptors_);
    if (!imgproc_ptr_->initialize()) { std::cerr << "Cannot initialize Image Processor..." << std::endl; return; }
    msckfvio_ptr_.reset(new cg::MsckfVio(calib, ekf));
    msckfvio_ptr_->attach(stream_);
    if (!msckfvio_ptr_->initialize()) { std::cerr << "Cannot initialize MsckfVio..." << std::endl; return; }
    ok_ = true;
}

System::~System() {
    imgproc_ptr_.reset();
    msckfvio_ptr_.reset();
    if (stream_) mskf_stream_destroy(stream_);
    if (own_ctx_) mskf_ctx_destroy(own_ctx_);
}

// system.cpp:40-43
void System::stereo_callback(const cg::Image &cam0_img, const cg::Image &cam1_img, bool is_draw) {
    if (!ok_) return;
    imgproc_ptr_->stereoCallback(cam0_img, cam1_img, is_draw);
    feature_msg_ptr_ = imgproc_ptr_->feature_msg_ptr_;
}

// system.cpp:45-48
void System::imu_callback(const cg::ImuConstPtr &msg) {
    if (!ok_) return;
    imgproc_ptr_->imuCallback(msg);
    msckfvio_ptr_->imuCallback(msg);
}

// system.cpp:50-54
void System::backend_callback() {
    if (!ok_) return;
    if (feature_msg_ptr_ == imgproc_ptr_->feature_msg_ptr_) msckfvio_ptr_->setZeroTailHint(feature_msg_ptr_.get(), imgproc_ptr_->zeroTailStart());
    msckfvio_ptr_->featureCallback(feature_msg_ptr_);
    if (copy_draw_buffers) {
        path_to_draw_ = msckfvio_ptr_->get_path();
        points3d_to_draw_ = msckfvio_ptr_->get_points3d();
    }
}

}  // namespace cg
