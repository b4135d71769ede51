// run_euroc_single_thread — headless counterpart of the reference harness apps/run_euroc_single_thread.cpp.
//
// Same argument (<path-to-euroc-mav0-dir>), same config path ("../config/camchain-imucam-euroc.yaml", Q16),
// same CSV parsing (timestamp = stoi(seconds)*1e9 + stoi(nanoseconds) in double, IMU values via stof; Q9),
// same call order per image: do { imu_callback } while (t_imu <= t_img); stereo_callback; backend_callback
// (reference :189-254, Q10).  No OpenCV / Pangolin: images are decoded by a small zlib-based reader of
// 8-bit grayscale PNG (what EuRoC ships) or binary PGM, and nothing is drawn (Q17).  Writes pose_out.txt.
// With "input_format" / "input_shift" in ../config/app_imgproc.yaml (this harness's own keys, mskf_fe_set_input_format) the
// reader also takes 16-bit grey PNG / PGM (TUM-VI), 8-bit RGB and RGBA PNG and binary PPM; a file whose pixel layout is not
// the one the configured format takes ends the run with an error and status 2.
// Options come from the YAML files, as in the reference.  One key of ../config/app_msckfvio.yaml is this harness's own:
// "covariance_out: <file>" also writes the covariance half of publish() (msckf_vio.cpp:1262-1293), one line per pose in the
// same std::fixed format: time stamp, the 36 entries of the 6x6 pose covariance, the 9 of the 3x3 velocity covariance
// (cg::System's YAML constructor switches MsckfVio::publishCovariance on).  Without the key nothing else is written.
#include <zlib.h>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../host/system.h"

static bool read_file(const std::string &path, std::vector<unsigned char> &buf) {
    std::ifstream f(path, std::ios::binary);
    if (!f.good()) return false;
    buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static unsigned be32(const unsigned char *p) { return (unsigned)p[0] << 24 | (unsigned)p[1] << 16 | (unsigned)p[2] << 8 | p[3]; }

// What an image file holds: its pixel layout, and the raw byte raster (rows = h, cols = w * bytes per pixel; 16-bit pixels
// in little-endian order, which is what the device reads: both file formats store them big-endian).
enum FileLayout { FILE_GRAY8 = 1, FILE_GRAY16 = 2, FILE_RGB8 = 3, FILE_RGBA8 = 4 };      // (the value is the bytes per pixel)
struct FileImage { int layout = 0; cg::YImg8 raw; };
static const char *layout_name(int layout) {
    return layout == FILE_GRAY8 ? "8-bit grey" : layout == FILE_GRAY16 ? "16-bit grey" : layout == FILE_RGB8 ? "8-bit RGB" : layout == FILE_RGBA8 ? "8-bit RGBA" : "nothing";
}
static void swap_pairs(unsigned char *p, size_t n_bytes) {
    for (size_t i = 0; i + 1 < n_bytes; i += 2) std::swap(p[i], p[i + 1]);
}

// non-interlaced PNG: 8-bit grey (colour type 0), 16-bit grey, 8-bit RGB (2), 8-bit RGBA (6)
static bool decode_png(const std::vector<unsigned char> &d, FileImage &out) {
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (d.size() < 33 || memcmp(d.data(), sig, 8) != 0) return false;
    size_t pos = 8;
    unsigned w = 0, h = 0, bpp = 0;
    std::vector<unsigned char> idat;
    while (pos + 12 <= d.size()) {
        const unsigned len = be32(&d[pos]);
        const std::string type((const char *)&d[pos + 4], 4);
        const unsigned char *body = &d[pos + 8];
        if (pos + 12 + len > d.size()) return false;
        if (type == "IHDR") {
            w = be32(body); h = be32(body + 4);
            const int depth = body[8], colour = body[9];
            if (depth == 8 && colour == 0) bpp = FILE_GRAY8;
            else if (depth == 16 && colour == 0) bpp = FILE_GRAY16;
            else if (depth == 8 && colour == 2) bpp = FILE_RGB8;
            else if (depth == 8 && colour == 6) bpp = FILE_RGBA8;
            if (!bpp || body[12] != 0) { std::cerr << "PNG: only non-interlaced 8-bit gray, 16-bit gray, 8-bit RGB and 8-bit RGBA are supported\n"; return false; }
        } else if (type == "IDAT") idat.insert(idat.end(), body, body + len);
        else if (type == "IEND") break;
        pos += 12 + len;
    }
    if (!w || !h || !bpp) return false;
    const size_t rb = (size_t)w * bpp;                // bytes of a row
    std::vector<unsigned char> raw((size_t)h * (rb + 1));
    uLongf rawlen = raw.size();
    if (uncompress(raw.data(), &rawlen, idat.data(), idat.size()) != Z_OK || rawlen != raw.size()) return false;
    out.layout = (int)bpp;
    out.raw = cg::YImg8((int)h, (int)rb);
    unsigned char *img = out.raw.data();
    for (unsigned y = 0; y < h; ++y) {
        const unsigned char ft = raw[(size_t)y * (rb + 1)];
        const unsigned char *src = &raw[(size_t)y * (rb + 1) + 1];
        unsigned char *row = img + (size_t)y * rb;
        const unsigned char *up = y ? row - rb : nullptr;
        for (size_t x = 0; x < rb; ++x) {              // the filters work on bytes, `bpp` bytes apart
            const int a = x >= bpp ? row[x - bpp] : 0, b = up ? up[x] : 0, c = (x >= bpp && up) ? up[x - bpp] : 0;
            int pred = 0;
            switch (ft) {
                case 0: pred = 0; break;
                case 1: pred = a; break;
                case 2: pred = b; break;
                case 3: pred = (a + b) >> 1; break;
                case 4: { const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
                default: return false;
            }
            row[x] = (unsigned char)(src[x] + pred);
        }
    }
    if (bpp == FILE_GRAY16) swap_pairs(img, (size_t)h * rb);
    return true;
}

// binary PGM (P5: maxval <= 255 8-bit, above 16-bit big-endian) and PPM (P6, maxval 255)
static bool decode_pnm(const std::vector<unsigned char> &d, FileImage &out) {
    if (d.size() < 15 || d[0] != 'P' || (d[1] != '5' && d[1] != '6')) return false;
    std::string hdr((const char *)d.data(), std::min<size_t>(d.size(), 64));
    std::istringstream ss(hdr);
    std::string magic; int w = 0, h = 0, mx = 0;
    ss >> magic >> w >> h >> mx;
    if (!ss.good() || w <= 0 || h <= 0) return false;
    const size_t off = (size_t)ss.tellg() + 1;
    int bpp;
    if (d[1] == '5') { if (mx < 1 || mx > 65535) return false; bpp = mx > 255 ? FILE_GRAY16 : FILE_GRAY8; if (bpp == FILE_GRAY8 && mx != 255) return false; }
    else { if (mx != 255) return false; bpp = FILE_RGB8; }
    const size_t bytes = (size_t)w * h * bpp;
    if (off + bytes > d.size()) return false;
    out.layout = bpp;
    out.raw = cg::YImg8(h, w * bpp);
    memcpy(out.raw.data(), d.data() + off, bytes);
    if (bpp == FILE_GRAY16) swap_pairs(out.raw.data(), bytes);
    return true;
}

static bool load_image(const std::string &path, FileImage &out) {
    std::vector<unsigned char> buf;
    if (!read_file(path, buf)) return false;
    return decode_png(buf, out) || decode_pnm(buf, out);
}

// the file layout the configured input format takes: a Bayer mosaic is an 8-bit grey file, bgr8 / bgra8 files have the
// layout of rgb8 / rgba8 ones
static int layout_of_format(int format) {
    switch (format) {
        case MSKF_PIX_GRAY16: return FILE_GRAY16;
        case MSKF_PIX_RGB8: case MSKF_PIX_BGR8: return FILE_RGB8;
        case MSKF_PIX_RGBA8: case MSKF_PIX_BGRA8: return FILE_RGBA8;
        default: return FILE_GRAY8;
    }
}

int main(int argc, char *argv[]) {
    if (argc != 2) {
        std::cout << "Arguments ERROR!" << std::endl;
        std::cout << "Usage: run_xxx <path-to-euroc-mav0-dir>" << std::endl;
        return -1;
    }
    const std::string euroc_dir = argv[1];
    const std::string file_cam_imu = "../config/camchain-imucam-euroc.yaml";
    const int num_cams = 2;
    cg::System system(file_cam_imu);
    if (!system.ok()) { std::cerr << "ERROR: cannot initialise the system (config files / GPU)" << std::endl; return -1; }

    const int input_format = system.imgproc_ptr_->inputFormat().format, want_layout = layout_of_format(input_format);

    // image masks (mask_cam0 / mask_cam1 / mask_margin of app_imgproc.yaml): 8-bit grey PNG or PGM of the calibration's size
    if (system.maskFiles().any()) {
        const cg::MaskFiles &mf = system.maskFiles();
        const std::string *const path[2] = {&mf.cam0, &mf.cam1};
        FileImage plane[2];
        int w = 0, h = 0;
        for (int c = 0; c < 2; ++c) {
            if (path[c]->empty()) continue;
            if (!load_image(*path[c], plane[c]) || plane[c].raw.empty()) { std::cerr << "ERROR: cannot read the mask " << *path[c] << std::endl; return 2; }
            if (plane[c].layout != FILE_GRAY8) { std::cerr << "ERROR: the mask " << *path[c] << " holds " << layout_name(plane[c].layout) << ", a mask is an 8-bit grey file" << std::endl; return 2; }
            const int pw = (int)plane[c].raw.cols(), ph = (int)plane[c].raw.rows();
            if (pw != system.imgproc_ptr_->imageWidth() || ph != system.imgproc_ptr_->imageHeight()) {
                std::cerr << "ERROR: the mask " << *path[c] << " is " << pw << " x " << ph << ", not the " << system.imgproc_ptr_->imageWidth() << " x "
                          << system.imgproc_ptr_->imageHeight() << " of the calibration" << std::endl;
                return 2;
            }
            w = pw; h = ph;
        }
        if (system.imgproc_ptr_->setMask(path[0]->empty() ? nullptr : plane[0].raw.data(), path[1]->empty() ? nullptr : plane[1].raw.data(), w, h, w, mf.margin) != MSKF_OK) {
            std::cerr << "ERROR: the masks " << mf.cam0 << " " << mf.cam1 << " were refused (mask_margin " << mf.margin << "): " << mskf_last_error() << std::endl;
            return 2;
        }
    }

    std::vector<std::vector<std::pair<double, std::string>>> data_img(num_cams);
    for (int n = 0; n < num_cams; ++n) {
        std::ifstream cam_file(euroc_dir + "/cam" + std::to_string(n) + "/data.csv");
        if (!cam_file.good()) { std::cerr << "ERROR: no cam file found !!!" << std::endl; return -1; }
        std::string line;
        std::getline(cam_file, line);
        while (std::getline(cam_file, line)) {
            std::stringstream stream(line);
            std::string s;
            std::getline(stream, s, ',');
            const std::string nanoseconds = s.substr(s.size() - 9, 9), seconds = s.substr(0, s.size() - 9);
            const double stamp_ns = std::stoi(seconds) * 1e9 + std::stoi(nanoseconds);
            std::getline(stream, s, ',');
            std::string imgname = s;
            while (!imgname.empty() && (imgname.back() == '\r' || imgname.back() == '\n' || imgname.back() == ' ')) imgname.pop_back();
            data_img[n].push_back(std::make_pair(stamp_ns, imgname));
        }
    }
    assert(data_img[0].size() == data_img[1].size());
    std::ifstream imu_file(euroc_dir + "/imu0/data.csv");
    if (!imu_file.good()) { std::cerr << "ERROR: no imu file found !!!" << std::endl; return -1; }
    std::string line;
    std::getline(imu_file, line);

    const size_t imgs_size = data_img[0].size();
    for (size_t idx_img = 0; idx_img < imgs_size; ++idx_img) {
        cg::Image imgs[2];
        bool ok = true;
        for (int j = 0; j < num_cams; ++j) {
            imgs[j].time_stamp = data_img[j][idx_img].first * 1e-9;
            const std::string img_path = euroc_dir + "/cam" + std::to_string(j) + "/data/" + data_img[j][idx_img].second;
            FileImage file;
            if (!load_image(img_path, file) || file.raw.empty()) { std::cerr << "ERROR: img is empty !!! " << img_path << std::endl; ok = false; continue; }
            if (file.layout != want_layout) {
                std::cerr << "ERROR: " << img_path << " holds " << layout_name(file.layout) << ", but input_format " << cg::input_format_name(input_format)
                          << " (app_imgproc.yaml) takes " << layout_name(want_layout) << " files" << std::endl;
                return 2;
            }
            imgs[j].image = std::move(file.raw);
        }
        if (!ok) return -1;
        const double t_img = imgs[0].time_stamp;
        double t_imu = 0.0;
        do {
            if (!std::getline(imu_file, line)) { t_imu = 1e300; break; }
            std::stringstream stream(line);
            std::string s;
            std::getline(stream, s, ',');
            const std::string nanoseconds = s.substr(s.size() - 9, 9), seconds = s.substr(0, s.size() - 9);
            const double stamp_ns = std::stoi(seconds) * 1e9 + std::stoi(nanoseconds);
            cg::Vector3 gyr, acc;
            for (int j = 0; j < 3; ++j) { std::getline(stream, s, ','); gyr[j] = std::stof(s); }
            for (int j = 0; j < 3; ++j) { std::getline(stream, s, ','); acc[j] = std::stof(s); }
            std::shared_ptr<cg::Imu> imu(new cg::Imu);
            imu->time_stamp = stamp_ns * 1e-9;
            imu->angular_velocity = gyr;
            imu->linear_acceleration = acc;
            system.imu_callback(imu);
            t_imu = imu->time_stamp;
        } while (t_imu <= t_img);
        system.stereo_callback(imgs[0], imgs[1], false);
        system.backend_callback();
    }
    std::cout << "done: " << imgs_size << " stereo frames, " << system.path_to_draw_.size() << " poses in pose_out.txt" << std::endl;
    return 0;
}
