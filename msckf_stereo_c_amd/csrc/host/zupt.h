// zupt.h — the stationarity test of the opt-in zero-velocity update: a pure function of the cam0 points of two consecutive
// feature messages.  Nothing but the standard library: the tests compile it with g++ alone.
//
// Points are the messages' undistorted NORMALISED cam0 coordinates, matched by feature id; fx, fy of cam0's calibration turn
// their differences into pixels.  Under quirk Q1 a message carries more than the current frame (stale records of earlier,
// longer frames behind the live ones, image_processor.cpp:1157-1164): the live records come first, so of every id its FIRST
// record is the current one and later records of the same id are skipped, in both messages.
//   n_common       = ids present in both messages
//   mean_disparity = sum over the common ids, in the order of the current message, of sqrt((fx du)^2 + (fy dv)^2), over n_common
//                    (0 when there is none)
// The pair is stationary when n_common >= min_features and mean_disparity < max_disparity.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zupt {

struct Point { uint64_t id; double u, v; };

struct Config {            // keys zupt, zupt_max_disparity, zupt_min_features, zupt_noise_std of app_msckfvio.yaml; absent: off.
    bool on = false;       // The three numbers are starting values nobody has tuned.
    double max_disparity = 0.5;     // pixels
    int min_features = 20;
    double noise_std = 0.05;        // m/s: R = noise_std^2 I of the zero-velocity measurement
};

struct Disparity { int n_common; double mean_disparity; };

// Open-addressing tables over the two messages' records (value = record index + 1, 0 = empty); a caller that tests every frame
// keeps one Scratch and so allocates nothing per frame.
struct Scratch { std::vector<uint32_t> prev_tab, curr_tab; };

namespace detail {
inline size_t table_size(size_t n) { size_t t = 16; while (t < 2 * n + 2) t <<= 1; return t; }
// index + 1 of the first record of `id` in the table, or 0; with `insert`, record i takes the free place (and 0 is returned)
inline uint32_t probe(std::vector<uint32_t> &tab, const Point *pts, uint64_t id, bool insert, size_t i) {
    const size_t mask = tab.size() - 1;
    for (size_t h = (size_t)((id * 0x9E3779B97F4A7C15ULL) >> 20) & mask;; h = (h + 1) & mask) {
        const uint32_t e = tab[h];
        if (e == 0) { if (insert) tab[h] = (uint32_t)i + 1; return 0; }
        if (pts[e - 1].id == id) return e;
    }
}
}  // namespace detail

inline Disparity disparity(const Point *prev, size_t n_prev, const Point *curr, size_t n_curr, double fx, double fy, Scratch *scratch = nullptr) {
    Scratch local;
    Scratch &sc = scratch ? *scratch : local;
    sc.prev_tab.assign(detail::table_size(n_prev), 0);
    sc.curr_tab.assign(detail::table_size(n_curr), 0);
    for (size_t i = 0; i < n_prev; ++i) detail::probe(sc.prev_tab, prev, prev[i].id, true, i);      // (a later record of an id finds the first and changes nothing)
    Disparity out{0, 0.0};
    double sum = 0.0;
    for (size_t i = 0; i < n_curr; ++i) {
        if (detail::probe(sc.curr_tab, curr, curr[i].id, true, i)) continue;                       // not the id's first record
        const uint32_t e = detail::probe(sc.prev_tab, prev, curr[i].id, false, 0);
        if (!e) continue;
        const double du = fx * (curr[i].u - prev[e - 1].u), dv = fy * (curr[i].v - prev[e - 1].v);
        sum += std::sqrt(du * du + dv * dv);
        ++out.n_common;
    }
    out.mean_disparity = out.n_common ? sum / (double)out.n_common : 0.0;
    return out;
}

inline bool stationary(const Disparity &d, const Config &c) { return d.n_common >= c.min_features && d.mean_disparity < c.max_disparity; }

}  // namespace zupt
