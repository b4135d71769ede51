// fe_book_scenarios.h — what the CPU checks of the front-end's device bookkeeping (msckf_stereo_c_amd/csrc/hip/fe_book.h) share:
// the random scenario generator (configurations, frames: track results, detector keys, the made-up outcome of the candidates'
// stereo match) and ref_frame, the plain restatement of the reference's own flow built on std::map and std::stable_sort
// (image_processor.cpp:416-513 trackFeatures tail, :622-756 addNewFeatures, :758-768 pruneGridFeatures; the same structure as
// oracle/o_frontend.cpp).  Used by fe_book_test.cpp (random frames, host run against ref_frame) and by
// fe_book_device_cases.cpp (named edge cases, host run against ref_frame, and the arenas the GPU test compares with).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "msckf_stereo_c_amd/csrc/hip/fe_book.h"

typedef unsigned long long u64;
struct Feat { u64 id = 0; float response = 0.f; int lifetime = 0; mskf_point2f cam0{0, 0}, cam1{0, 0}, und0{0, 0}, und1{0, 0}; };
typedef std::map<int, std::vector<Feat>> Grid;

struct Cfg { int W, H, grid_row, grid_col, grid_min, grid_max, det_rows, det_cols, thr, q4; int ransac; double K[2][4], R[2][9], ransac_thr; };

// the product's host implementation of twoPointRansac (csrc/host/image_processor.cpp; == the oracle's, tests/test_ransac.py)
extern "C" void mskfh_two_point_ransac(int n, const mskf_point2f *pts1_und, const mskf_point2f *pts2_und, const double *R_p_c, const double *intrinsics,
                                       double inlier_error, double success_probability, unsigned long long *draws, int32_t *markers);
struct Info { int before = 0, after_tracking = 0, after_matching = 0, after_ransac = 0; };

static unsigned hash2(float x, float y, unsigned salt) {
    unsigned a, b;
    std::memcpy(&a, &x, 4); std::memcpy(&b, &y, 4);
    unsigned h = a * 2654435761u ^ (b + salt) * 40503u;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    return h;
}
// a case may decide the stereo outcome of its candidates itself (all fail, all pass, ...): bit 1 of what this returns
static int (*g_cand_status_hook)(mskf_point2f p, unsigned salt) = nullptr;
// the (made-up, deterministic) outcome of the stereo match of a candidate point
static void cand_result(mskf_point2f p, unsigned salt, mskf_point2f &o1, mskf_point2f &u0, mskf_point2f &u1, uint8_t &status) {
    const unsigned h = hash2(p.x, p.y, salt);
    status = (uint8_t)(1 | ((h % 10) < 7 ? 2 : 0));
    if (g_cand_status_hook) status = (uint8_t)(1 | (g_cand_status_hook(p, salt) ? 2 : 0));
    o1 = mskf_point2f{p.x - 3.25f - (float)(h & 7), p.y + 0.5f};
    u0 = mskf_point2f{p.x * 0.002f - 0.7f, p.y * 0.002f - 0.4f};
    u1 = mskf_point2f{o1.x * 0.002f - 0.7f, o1.y * 0.002f - 0.4f};
}

struct Frame {      // the inputs of one frame
    std::vector<mskf_point2f> t_out0, t_out1, t_und0, t_und1;
    std::vector<uint8_t> t_status;
    std::vector<u64> keys;
    unsigned gen, salt;
};

// ---------------------------------------------------------------------------------------------- reference flow
static void ref_frame(const Cfg &c, const Frame &f, const Grid &prev, Grid &curr, Info &info, u64 &next_id, u64 &ransac_draws,
                      std::vector<mskf_point2f> &cand_sent, std::vector<int> &cand_sent_index) {
    const int grid_height = c.H / c.grid_row, grid_width = c.W / c.grid_col;
    const int det_ch = (c.H + c.det_rows - 1) / c.det_rows, det_cw = (c.W + c.det_cols - 1) / c.det_cols;
    const int n_cells = c.grid_row * c.grid_col;
    curr.clear();
    // trackFeatures (:352-513) after the tracks
    std::vector<Feat> flat;
    for (const auto &it : prev) for (const auto &pf : it.second) flat.push_back(pf);
    info.before = (int)flat.size();
    if (!flat.empty()) {
        info.after_tracking = info.after_matching = info.after_ransac = 0;
        // :482-500 (Q5 cleared): the matched cam0 and cam1 pairs through twoPointRansac, a feature must be an inlier of both
        std::vector<int> keep(flat.size(), 1);
        if (c.ransac) {
            std::vector<size_t> idx;
            std::vector<mskf_point2f> p0, c0, p1, c1;
            for (size_t i = 0; i < flat.size(); ++i) {
                if ((f.t_status[i] & 3) != 3) continue;
                idx.push_back(i);
                p0.push_back(flat[i].und0); p1.push_back(flat[i].und1); c0.push_back(f.t_und0[i]); c1.push_back(f.t_und1[i]);
            }
            std::vector<int32_t> in0(idx.size() + 1), in1(idx.size() + 1);
            mskfh_two_point_ransac((int)idx.size(), p0.data(), c0.data(), c.R[0], c.K[0], c.ransac_thr, 0.99, &ransac_draws, in0.data());
            mskfh_two_point_ransac((int)idx.size(), p1.data(), c1.data(), c.R[1], c.K[1], c.ransac_thr, 0.99, &ransac_draws, in1.data());
            for (size_t k = 0; k < idx.size(); ++k) keep[idx[k]] = in0[k] != 0 && in1[k] != 0;
        }
        for (size_t i = 0; i < flat.size(); ++i) {
            if (!(f.t_status[i] & 1)) continue;
            ++info.after_tracking;
            if (!(f.t_status[i] & 2)) continue;
            ++info.after_matching;
            if (!keep[i]) continue;
            const int row = static_cast<int>(f.t_out0[i].y / grid_height), col = static_cast<int>(f.t_out0[i].x / grid_width);
            const int code = row * c.grid_col + col;
            Feat g = flat[i];
            g.lifetime = flat[i].lifetime + 1;
            g.response = 0.f;
            g.cam0 = f.t_out0[i]; g.cam1 = f.t_out1[i]; g.und0 = f.t_und0[i]; g.und1 = f.t_und1[i];
            curr[code].push_back(g);
            ++info.after_ransac;
        }
    }
    // addNewFeatures (:622-756)
    std::vector<uint8_t> occ((size_t)c.det_rows * c.det_cols, 0);
    for (const auto &it : curr)
        for (const auto &ft : it.second) {
            const int y = static_cast<int>(ft.cam0.y), x = static_cast<int>(ft.cam0.x);
            int r = (int)((float)y / (float)det_ch), cc = (int)((float)x / (float)det_cw);
            r = r < 0 ? 0 : (r >= c.det_rows ? c.det_rows - 1 : r);
            cc = cc < 0 ? 0 : (cc >= c.det_cols ? c.det_cols - 1 : cc);
            occ[(size_t)r * c.det_cols + cc] = 1;
        }
    std::vector<mskf_point2f> new_features;
    std::vector<double> new_features_responses;
    for (int k = 0; k < c.det_rows * c.det_cols; ++k) {
        const u64 key = f.keys[k];
        if ((unsigned)(key >> 56) != f.gen) continue;
        const int score = (int)((key >> 32) & 0xFFFFFFULL);
        if (score <= c.thr || occ[k]) continue;
        const unsigned order = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFULL);
        const int cy = k / c.det_cols, cx = k - cy * c.det_cols;
        new_features.push_back(mskf_point2f{(float)(cx * det_cw + (int)(order % (unsigned)det_cw)), (float)(cy * det_ch + (int)(order / (unsigned)det_cw))});
        new_features_responses.push_back((double)score / 256.0);
    }
    std::vector<std::vector<std::pair<mskf_point2f, double>>> sieve((size_t)n_cells);
    for (size_t i = 0; i < new_features.size(); ++i) {
        const int row = static_cast<int>(new_features[i].y / grid_height), col = static_cast<int>(new_features[i].x / grid_width);
        const size_t code = (size_t)(row * c.grid_col + col);
        if (code >= sieve.size()) continue;
        sieve[code].push_back(std::make_pair(new_features[i], new_features_responses[i]));
    }
    std::vector<mskf_point2f> cand;
    std::vector<double> sieved_responses;
    std::vector<int> cand_code;
    for (size_t code = 0; code < sieve.size(); ++code) {
        auto &item = sieve[code];
        if ((int)item.size() > c.grid_max) {
            std::stable_sort(item.begin(), item.end(), [](const std::pair<mskf_point2f, double> &a, const std::pair<mskf_point2f, double> &b) { return a.second > b.second; });
            item.erase(item.begin() + c.grid_max, item.end());
        }
        for (const auto &p : item) { cand.push_back(p.first); sieved_responses.push_back(p.second); cand_code.push_back((int)code); }
    }
    // what the device sends to the second track call: the candidates of the cells with a vacancy, with their position in this list
    cand_sent.clear(); cand_sent_index.clear();
    for (size_t i = 0; i < cand.size(); ++i) {
        const int have = curr.count(cand_code[i]) ? (int)curr[cand_code[i]].size() : 0;
        if (have < c.grid_min) { cand_sent.push_back(cand[i]); cand_sent_index.push_back((int)i); }
    }
    std::map<int, std::vector<Feat>> grid_new;
    for (int code = 0; code < n_cells; ++code) grid_new[code] = std::vector<Feat>();
    for (size_t i = 0; i < cand.size(); ++i) {
        mskf_point2f o1, u0, u1; uint8_t st;
        cand_result(cand[i], f.salt, o1, u0, u1, st);
        if (!(st & 2)) continue;
        Feat nf;
        nf.response = (float)(c.q4 ? new_features_responses[i] : sieved_responses[i]);      // Q4 (:698)
        nf.cam0 = cand[i]; nf.cam1 = o1; nf.und0 = u0; nf.und1 = u1;
        const int row = static_cast<int>(cand[i].y / grid_height), col = static_cast<int>(cand[i].x / grid_width);
        grid_new[row * c.grid_col + col].push_back(nf);
    }
    for (auto &it : grid_new) std::stable_sort(it.second.begin(), it.second.end(), [](const Feat &a, const Feat &b) { return a.response > b.response; });
    for (int code = 0; code < n_cells; ++code) {
        std::vector<Feat> &here = curr[code];
        std::vector<Feat> &fresh = grid_new[code];
        if ((int)here.size() >= c.grid_min) continue;
        const int vacancy = c.grid_min - (int)here.size();
        for (int k = 0; k < vacancy && k < (int)fresh.size(); ++k) {
            here.push_back(fresh[k]);
            here.back().id = next_id++;
            here.back().lifetime = 1;
        }
    }
    // pruneGridFeatures (:758-768)
    for (auto &it : curr) {
        auto &g = it.second;
        if ((int)g.size() <= c.grid_max) continue;
        std::stable_sort(g.begin(), g.end(), [](const Feat &a, const Feat &b) { return a.lifetime > b.lifetime; });
        g.erase(g.begin() + c.grid_max, g.end());
    }
}


// ---------------------------------------------------------------------------------------------- scenario generator
// (the order of the draws is part of it: fe_book_test's summary line counts what these scenarios contain)
template <class Rng> static int rnd_int(Rng &rng, int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; }

// a random configuration; every other trial runs the 2-point RANSAC
template <class Rng> static void gen_cfg(Rng &rng, int trial, Cfg &c) {
    auto U = [&](int lo, int hi) { return rnd_int(rng, lo, hi); };
    const int sizes[][2] = {{752, 480}, {376, 240}, {333, 251}, {1280, 720}, {640, 400}};
    const int si = U(0, 4);
    c.W = sizes[si][0]; c.H = sizes[si][1];
    c.grid_row = U(2, 10); c.grid_col = U(2, 12);
    c.grid_min = U(1, 6); c.grid_max = c.grid_min + U(0, 3);
    c.det_rows = 30; c.det_cols = 47;
    c.thr = 10 * 256; c.q4 = U(0, 1);
    // every other trial runs the 2-point RANSAC between the tracks: cameras with EuRoC-like focal lengths, a small rotation
    c.ransac = trial & 1; c.ransac_thr = 3.0;
    for (int cam = 0; cam < 2; ++cam) {
        c.K[cam][0] = 458.654 - 1.2 * cam; c.K[cam][1] = 457.296 - 0.8 * cam; c.K[cam][2] = 367.215; c.K[cam][3] = 248.375;
        const double wx = 1e-3 * U(-5, 5), wy = 1e-3 * U(-5, 5), wz = 1e-3 * U(-5, 5);
        const double Rm[9] = {1.0, -wz, wy, wz, 1.0, -wx, -wy, wx, 1.0};
        std::memcpy(c.R[cam], Rm, sizeof(Rm));
    }
}

// the random inputs of frame `fr`: `flat` is the previous grid in flatten order
template <class Rng> static void gen_frame(Rng &rng, const Cfg &c, int fr, const std::vector<Feat> &flat, Frame &f) {
    auto U = [&](int lo, int hi) { return rnd_int(rng, lo, hi); };
    const int grid_w = c.W / c.grid_col;
    const int det_ch = (c.H + c.det_rows - 1) / c.det_rows, det_cw = (c.W + c.det_cols - 1) / c.det_cols;
    const int det_cells = c.det_rows * c.det_cols;
    const int n = (int)flat.size();
    f.gen = (unsigned)(fr % 255) + 1; f.salt = rng();
    const int loss = U(0, 100);       // percent of the features this frame loses (some frames lose everything)
    // RANSAC trials: the undistorted points move by a common flow (0: pure rotation, the degenerate branch) plus noise, a
    // few of them wildly; otherwise they are unrelated to the previous frame's
    const float flow_x = c.ransac ? 0.0011f * (float)U(-4, 4) : 0.f, flow_y = c.ransac ? 0.0009f * (float)U(-4, 4) : 0.f;
    f.t_out0.resize(n); f.t_out1.resize(n); f.t_und0.resize(n); f.t_und1.resize(n); f.t_status.resize(n);
    for (int i = 0; i < n; ++i) {
        const int r = U(0, 99);
        f.t_status[i] = (uint8_t)(r < loss / 2 ? 0 : (r < loss ? 1 : 3));
        const int kind = U(0, 19);
        float x = (float)U(0, c.W - 2) + (float)U(0, 1023) / 1024.f, y = (float)U(0, c.H - 2) + (float)U(0, 1023) / 1024.f;
        if (kind == 0) x = (float)(c.W - 1);
        if (kind == 1) y = (float)(c.H - 1);
        if (kind == 2) { x = 0.f; y = 0.f; }
        if (kind == 3) x = (float)(c.grid_col * grid_w) + 0.25f < (float)(c.W - 1) ? (float)(c.grid_col * grid_w) + 0.25f : x;   // Q7: column == grid_col
        f.t_out0[i] = mskf_point2f{x, y};
        f.t_out1[i] = mskf_point2f{x - 5.5f, y + 0.125f};
        f.t_und0[i] = mskf_point2f{x * 0.001f, y * 0.001f};
        f.t_und1[i] = mskf_point2f{x * 0.001f - 0.01f, y * 0.001f};
        if (c.ransac) {
            const float wild = U(0, 9) == 0 ? 0.02f * (float)U(-3, 3) : 0.f;
            const float zx = flat[i].und0.x * 0.1f * (float)U(0, 3) * flow_x, zy = flat[i].und0.y * 0.1f * (float)U(0, 3) * flow_y;    // depth-like spread along the flow
            f.t_und0[i] = mskf_point2f{flat[i].und0.x + flow_x + zx + 1e-5f * (float)U(-20, 20) + wild, flat[i].und0.y + flow_y + zy + 1e-5f * (float)U(-20, 20)};
            f.t_und1[i] = mskf_point2f{flat[i].und1.x + flow_x + zx + 1e-5f * (float)U(-20, 20), flat[i].und1.y + flow_y + zy + 1e-5f * (float)U(-20, 20) - wild};
        }
        if (f.t_status[i] != 3) { f.t_out1[i] = mskf_point2f{0, 0}; }
    }
    f.keys.assign(det_cells, 0ULL);
    const int density = U(0, 100);
    for (int k = 0; k < det_cells; ++k) {
        if (U(0, 99) >= density) continue;
        const int cy = k / c.det_cols, cx = k - cy * c.det_cols;
        const int x0 = cx * det_cw, y0 = cy * det_ch;
        if (x0 >= c.W || y0 >= c.H) continue;
        const int ox = U(0, std::min(det_cw, c.W - x0) - 1), oy = U(0, std::min(det_ch, c.H - y0) - 1);
        const unsigned order = (unsigned)(oy * det_cw + ox);
        const int score = U(0, 3) == 0 ? c.thr + U(-2, 2) : c.thr + 256 * U(1, 6);       // few distinct values: ties everywhere
        const unsigned gen = U(0, 9) == 0 ? ((f.gen + 7) % 255) + 1 : f.gen;           // some keys are stale
        f.keys[k] = ((u64)gen << 56) | ((u64)(unsigned)score << 32) | (0xFFFFFFFFu - order);
    }
}
