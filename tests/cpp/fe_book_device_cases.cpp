// fe_book_device_cases.cpp — the named edge cases of the front-end's bookkeeping (msckf_stereo_c_amd/csrc/hip/fe_book.h) as a
// small shared library for tests/test_fe_book_cases.py (CPU) and tests/test_gpu_fe_book.py (k_fe_book on the device).
//
// A case is a configuration, an optional seeded previous grid and 3-8 frames of inputs.  Everything a FeBookDev points to
// lies in ONE arena (fbc_carve, in the manner of book_carve in mskf_capi_fe.cpp): the same routine gives the size on a null
// base and fills a descriptor for any base, host or device.  The arena is filled with a fixed pattern before anything is
// written, so the unused tail of every array is a canary.  Per frame the helper writes the inputs (snapshot 0), runs
// fe_book1 of the header's host branch (snapshot 1), writes the candidates' stereo results (snapshot 2), runs fe_book2
// (snapshot 3), and runs ref_frame (fe_book_scenarios.h) beside it.  The GPU test uploads the same inputs, launches
// k_fe_book and compares whole arenas with snapshots 1 and 3, byte for byte.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -Wall -Werror -shared -fPIC [-DFB_HOST_ORDER=1|2] -I<repo>
//        tests/cpp/fe_book_device_cases.cpp -lmskf_host -lmskf_hip
#include <cmath>
#include <set>
#include <string>
#include <utility>
#include "fe_book_scenarios.h"

namespace {

const unsigned char FILL = 0x5a;

struct Arr { const char *name; size_t off, bytes, elem; };

// ONE sequence of take()s for everything a FeBookDev points to; every region rounded up to 256 bytes.  D holds the
// capacities and the grid / detector geometry on entry.  grid[0], grid[1] are the two published grids (prev / curr swap per
// frame), grid[2] the tracked list.  [in_lo, in_hi) are the inputs of fe_book1 (the results of the first track call and the
// cell keys), [c_lo, c_hi) those of fe_book2 (the results of the second track call).
struct Carved { FeGridArr grid[3]; size_t in_lo, in_hi, c_lo, c_hi, size; };
size_t fbc_carve(char *base, FeBookDev &D, Carved &K, std::vector<Arr> *tab) {
    size_t off = 0;
    auto take = [&](auto *&p, size_t count, const char *name) {
        typedef std::remove_cv_t<std::remove_reference_t<decltype(*p)>> T;
        p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + off);
        if (tab) tab->push_back(Arr{name, off, sizeof(T) * count, sizeof(T)});
        off += (sizeof(T) * count + 255) & ~(size_t)255;
    };
    const size_t cap = (size_t)D.cap, cand_cap = (size_t)D.cand_cap, det_cap = (size_t)D.det_cap;
    take(D.st, 1, "state");
    static const char *const gname[3][8] = {
        {"grid0.id", "grid0.lifetime", "grid0.code", "grid0.response", "grid0.cam0", "grid0.cam1", "grid0.und0", "grid0.und1"},
        {"grid1.id", "grid1.lifetime", "grid1.code", "grid1.response", "grid1.cam0", "grid1.cam1", "grid1.und0", "grid1.und1"},
        {"tracked.id", "tracked.lifetime", "tracked.code", "tracked.response", "tracked.cam0", "tracked.cam1", "tracked.und0", "tracked.und1"}};
    for (int g = 0; g < 3; ++g) {
        FeGridArr &G = K.grid[g];
        take(G.id, cap, gname[g][0]); take(G.lifetime, cap, gname[g][1]); take(G.code, cap, gname[g][2]); take(G.response, cap, gname[g][3]);
        take(G.cam0, cap, gname[g][4]); take(G.cam1, cap, gname[g][5]); take(G.und0, cap, gname[g][6]); take(G.und1, cap, gname[g][7]);
    }
    D.tracked = K.grid[2];
    take(D.det_pt, det_cap, "det_pt"); take(D.det_score, det_cap, "det_score");
    take(D.cand_pt, cand_cap, "cand_pt"); take(D.cand_index, cand_cap, "cand_index"); take(D.cand_score, cand_cap, "cand_score");
    take(D.cand_off, (size_t)D.n_cells + 1, "cand_off"); take(D.cand_cnt, (size_t)D.n_cells + 1, "cand_cnt");
    take(D.cell_count, (size_t)D.n_codes + 1, "cell_count");
    K.in_lo = off;
    take(D.t_out0, cap, "t_out0"); take(D.t_out1, cap, "t_out1"); take(D.t_und0, cap, "t_und0"); take(D.t_und1, cap, "t_und1"); take(D.t_status, cap, "t_status");
    take(D.cell_keys, det_cap, "cell_keys");
    K.in_hi = K.c_lo = off;
    take(D.c_out0, cand_cap, "c_out0"); take(D.c_out1, cand_cap, "c_out1"); take(D.c_und0, cand_cap, "c_und0"); take(D.c_und1, cand_cap, "c_und1");
    take(D.c_status, cand_cap, "c_status");
    K.c_hi = off;
    take(D.rs_pair, 4 * cap, "rs_pair"); take(D.rs_pt, 4 * cap, "rs_pt"); take(D.rs_scalar, 48, "rs_scalar");
    // the export block, through the header's own definition
    FeExport x;
    const size_t xb = fe_book_export((char *)((uintptr_t)base + off), D.cap, x);
    D.x_info = x.info; D.x_id = x.id; D.x_lifetime = x.lifetime; D.x_cam0 = x.cam0; D.x_cam1 = x.cam1; D.x_und0 = x.und0; D.x_und1 = x.und1;
    if (tab) {
        auto at = [&](const void *p) { return (size_t)((uintptr_t)p - (uintptr_t)base); };
        tab->push_back(Arr{"x_info", at(x.info), sizeof(int) * FX_WORDS, sizeof(int)});
        tab->push_back(Arr{"x_id", at(x.id), sizeof(unsigned long long) * cap, sizeof(unsigned long long)});
        tab->push_back(Arr{"x_lifetime", at(x.lifetime), sizeof(int) * cap, sizeof(int)});
        tab->push_back(Arr{"x_cam0", at(x.cam0), sizeof(mskf_point2f) * cap, sizeof(mskf_point2f)});
        tab->push_back(Arr{"x_cam1", at(x.cam1), sizeof(mskf_point2f) * cap, sizeof(mskf_point2f)});
        tab->push_back(Arr{"x_und0", at(x.und0), sizeof(mskf_point2f) * cap, sizeof(mskf_point2f)});
        tab->push_back(Arr{"x_und1", at(x.und1), sizeof(mskf_point2f) * cap, sizeof(mskf_point2f)});
    }
    off += (xb + 255) & ~(size_t)255;
    K.size = off;
    return off;
}

// ---------------------------------------------------------------------------------------------- cases
struct FrameSpec {
    int keep = -1;          // previous features that keep status 3, spread over the list (-1: all)
    int lost = -1;          // status of the others: 0, 1, or -1: alternating
    int place = 0;          // 0: where the feature was; 1: anywhere, with the generator's border kinds; 2: all into the cell
                            // of code 7 of the 4 x 5 grid on 376 x 240; 3: the last row / column and the partial ones (Q7)
    int und = 0;            // 0: unrelated to the previous frame's; 1: previous + flow + depth spread + noise; 2: previous + a
                            // random displacement below the 50 npu gate
    float flow_x = 0.f, flow_y = 0.f;
    int wild_both = 0;      // und 1: all but this many of the kept features jump by 0.3 in both cameras (0: nobody jumps)
    int wild1_pct = 0;      // und 1: percent of the features whose cam1 point alone leaves the model
    int density = 0;        // percent of the detector cells that hold a key
    int same_score = 0;     // every key has the same score
    int stale_pct = 0;      // percent of the keys that carry another generation
    int cand = 0;           // stereo outcome of the candidates: 0: the generator's hash, 1: all fail, 2: all pass, 3: only the
                            // last candidate of each cell passes
};
struct Case {
    std::string set, name;
    Cfg c;
    int seed_n = 0;         // features of the previous grid of frame 0, written into the arena directly
    int seed_mode = 0;      // 0: round-robin over the nominal cells; 1: one per detector cell
    int life_mode = 0;      // lifetimes of the seeded features: 0: varied, 1: all equal, 2: four tied groups
    std::vector<FrameSpec> frames;
    int random_trial = -1;  // >= 0: the frames of the random generator
};

Cfg base_cfg(int W, int H, int grid_row, int grid_col, int grid_min, int grid_max) {
    Cfg c;
    c.W = W; c.H = H; c.grid_row = grid_row; c.grid_col = grid_col; c.grid_min = grid_min; c.grid_max = grid_max;
    c.det_rows = 30; c.det_cols = 47; c.thr = 10 * 256; c.q4 = 1; c.ransac = 0; c.ransac_thr = 3.0;
    for (int cam = 0; cam < 2; ++cam) {
        c.K[cam][0] = 458.654 - 1.2 * cam; c.K[cam][1] = 457.296 - 0.8 * cam; c.K[cam][2] = 367.215; c.K[cam][3] = 248.375;
        const double w = 1e-4 * (cam + 1);
        const double Rm[9] = {1.0, -w, 2 * w, w, 1.0, -3 * w, -2 * w, 3 * w, 1.0};
        std::memcpy(c.R[cam], Rm, sizeof(Rm));
    }
    return c;
}
FrameSpec fs(int keep, int place, int density) { FrameSpec f; f.keep = keep; f.place = place; f.density = density; return f; }

std::vector<Case> make_cases() {
    std::vector<Case> v;
    auto add = [&](const char *set, const std::string &name, const Cfg &c, int seed_n, std::vector<FrameSpec> frames) -> Case & {
        Case k; k.set = set; k.name = name; k.c = c; k.seed_n = seed_n; k.frames = std::move(frames);
        v.push_back(k);
        return v.back();
    };
    // ---- item counts around the wavefront and the workgroup: 12 x 8 grid, grid_min = grid_max = 6, cap 584.  Frame 0 has
    //      n_prev = N (seeded) and tracks the next smaller count, which is the n_prev of frame 1, and so on; no detector keys
    //      until the last frame, which refills the grid
    const int counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513};
    for (int k = 0; k < 11; ++k) {
        const Cfg c = base_cfg(376, 240, 12, 8, 6, 6);
        add("counts", "n_prev_" + std::to_string(counts[k]), c, counts[k],
            {fs(k >= 1 ? counts[k - 1] : 0, 0, 0), fs(k >= 2 ? counts[k - 2] : 0, 0, 0), fs(k >= 3 ? counts[k - 3] : 0, 1, 60), fs(-1, 1, 30)});
    }
    // ---- the short-list bounds
    {
        const int b[4][2] = {{16, 16}, {0, 0}, {0, 3}, {1, 16}};
        for (int k = 0; k < 4; ++k) {
            const Cfg c = base_cfg(376, 240, 4, 5, b[k][0], b[k][1]);
            add("bounds", "grid_" + std::to_string(b[k][0]) + "_" + std::to_string(b[k][1]), c, k == 0 || k == 3 ? 0 : 12,
                {fs(8, 1, 100), fs(-1, 0, 100), fs(-1, 1, 70), fs(-1, 2, 100)});
        }
    }
    // ---- one crowded cell: 300 survivors tracked into one grid code
    for (int k = 0; k < 2; ++k) {
        const Cfg c = base_cfg(376, 240, 4, 5, 4, 16);
        Case &cs = add("crowded", k == 0 ? "crowded_equal_lifetimes" : "crowded_tied_lifetimes", c, 300, {fs(-1, 2, 50), fs(-1, 0, 100), fs(-1, 2, 100)});
        cs.life_mode = k + 1;
    }
    // ---- ties: every key the same score, so every candidate the same response, under both settings of Q4
    for (int q4 = 0; q4 < 2; ++q4) {
        Cfg c = base_cfg(376, 240, 4, 5, 3, 4);
        c.q4 = q4;
        std::vector<FrameSpec> fr = {fs(0, 1, 100), fs(6, 1, 100), fs(10, 1, 80)};
        for (auto &f : fr) f.same_score = 1;
        add("ties", std::string("ties_q4_") + (q4 ? "on" : "off"), c, 0, fr);
    }
    // ---- detector extremes
    {
        const Cfg c = base_cfg(376, 240, 4, 5, 3, 4);
        add("detector", "det_no_key", c, 40, {fs(30, 1, 0), fs(-1, 1, 0), fs(-1, 0, 0)});
        add("detector", "det_every_cell", c, 0, {fs(-1, 0, 100), fs(0, 0, 100), fs(-1, 1, 100)});
        const Cfg f = base_cfg(376, 240, 10, 12, 3, 16);
        Case &occ = add("detector", "det_every_cell_occupied", f, 1410, {fs(-1, 0, 100), fs(-1, 0, 100), fs(-1, 1, 100)});
        occ.seed_mode = 1;
        std::vector<FrameSpec> st = {fs(-1, 0, 100), fs(0, 0, 100), fs(-1, 1, 100)};
        for (auto &x : st) x.stale_pct = 50;
        add("detector", "det_half_stale", c, 0, st);
    }
    // ---- candidates
    for (int k = 1; k <= 3; ++k) {
        const Cfg c = base_cfg(376, 240, 4, 5, 3, 4);
        std::vector<FrameSpec> fr = {fs(-1, 0, 100), fs(5, 1, 100), fs(10, 1, 100)};
        for (auto &x : fr) x.cand = k;
        add("candidates", k == 1 ? "cand_all_fail" : (k == 2 ? "cand_all_pass" : "cand_last_of_cell"), c, k == 1 ? 20 : 0, fr);
    }
    // ---- Q7 geometry: partial rows and columns
    {
        add("q7", "q7_333x251_4x5", base_cfg(333, 251, 4, 5, 3, 4), 0, {fs(-1, 0, 100), fs(-1, 3, 100), fs(-1, 3, 50), fs(-1, 1, 100)});
        add("q7", "q7_333x251_3x7", base_cfg(333, 251, 3, 7, 2, 5), 0, {fs(-1, 0, 100), fs(-1, 3, 100), fs(-1, 3, 50), fs(-1, 1, 100)});
    }
    // ---- RANSAC branches
    {
        Cfg c = base_cfg(376, 240, 12, 8, 6, 6);
        c.ransac = 1;
        auto flow = [](int keep, int density) { FrameSpec f = fs(keep, 0, density); f.und = 1; f.flow_x = 0.0044f; f.flow_y = -0.0027f; f.lost = 1; return f; };
        const int nm[] = {0, 1, 2, 3, 64, 257};
        for (int k = 0; k < 6; ++k) add("ransac", "ransac_n_match_" + std::to_string(nm[k]), c, 300, {flow(nm[k], 100), flow(-1, 50), flow(-1, 50)});
        FrameSpec gate = flow(50, 100); gate.wild_both = 2;
        add("ransac", "ransac_gate_leaves_2", c, 300, {gate, flow(-1, 50), gate});
        FrameSpec rot = flow(-1, 50); rot.flow_x = rot.flow_y = 0.f;
        add("ransac", "ransac_pure_rotation", c, 300, {rot, rot, rot});
        FrameSpec none = flow(120, 50); none.und = 2;
        add("ransac", "ransac_no_hypothesis", c, 300, {none, flow(-1, 50), none});
        add("ransac", "ransac_clean_translation", c, 300, {flow(-1, 50), flow(-1, 50), flow(-1, 50)});
        FrameSpec c1 = flow(-1, 50); c1.wild1_pct = 30;
        add("ransac", "ransac_cam1_rejects", c, 300, {c1, c1, c1});
    }
    // ---- more than 64 KiB of LDS
    {
        Cfg c = base_cfg(1280, 720, 10, 12, 4, 16);
        c.det_rows = 60; c.det_cols = 94;
        add("lds", "lds_over_64k", c, 0, {fs(-1, 0, 100), fs(-1, 1, 100), fs(600, 1, 60)});
    }
    // ---- random: the generator of fe_book_test with grid_min / grid_max over 0..16
    for (int t = 0; t < 40; ++t) {
        Case k;
        k.set = "random" + std::to_string(t / 10); k.name = "random_" + std::to_string(t); k.random_trial = t;
        v.push_back(k);
    }
    return v;
}

const std::vector<Case> &cases() { static const std::vector<Case> v = make_cases(); return v; }

// ---------------------------------------------------------------------------------------------- one case, run on the host
enum { CE_N_PREV, CE_N_TRACKED, CE_N_DET, CE_N_CAND, CE_N_NEW, CE_N_CURR, CE_DRAWS, CE_OVERFLOW, CE_BEFORE, CE_AFTER_TRACKING, CE_AFTER_MATCHING,
       CE_AFTER_RANSAC, CE_MAX_TRACKED_CELL, CE_MAX_CURR_CELL, CE_MAX_CODE, CE_N_CELLS, CE_CELLS_WITH_CAND, CE_SCORE_LO, CE_SCORE_HI, CE_IN0, CE_IN1,
       CE_MAX_DET_CELL, CE_NAN_WORDS, CE_KEYS, CE_GRID_MAX, CE_WORDS };

struct Run {
    const Case *cs = nullptr;
    Cfg c;
    FeBookDev D;                        // the constant part (pointers: those of the host arena)
    Carved K;
    std::vector<Arr> tab;
    size_t scratch_bytes = 0;
    std::vector<char> init;             // the arena before the first frame
    std::vector<std::vector<char>> snap;    // 4 per frame
    std::vector<unsigned> gen;          // per frame
    std::vector<int> census;            // CE_WORDS per frame
    std::string error;                  // a difference from ref_frame, or empty
};

std::set<std::pair<unsigned, unsigned>> g_pass;     // cand mode 3: the points that pass
int g_cand_mode = 0;
std::pair<unsigned, unsigned> bits_of(mskf_point2f p) { unsigned a, b; std::memcpy(&a, &p.x, 4); std::memcpy(&b, &p.y, 4); return std::make_pair(a, b); }
int cand_hook(mskf_point2f p, unsigned) { return g_cand_mode == 1 ? 0 : (g_cand_mode == 2 ? 1 : (g_pass.count(bits_of(p)) ? 1 : 0)); }

bool same_pt(mskf_point2f a, mskf_point2f b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

struct Dims { int grid_h, grid_w, det_ch, det_cw, n_cells, n_codes, det_cells, cap, cand_cap, det_cap; };
// the capacities as book_alloc (mskf_capi_fe.cpp) derives them
Dims dims_of(const Cfg &c) {
    Dims d;
    d.grid_h = c.H / c.grid_row; d.grid_w = c.W / c.grid_col;
    d.det_ch = (c.H + c.det_rows - 1) / c.det_rows; d.det_cw = (c.W + c.det_cols - 1) / c.det_cols;
    d.n_cells = c.grid_row * c.grid_col;
    d.n_codes = std::max(((c.H - 1) / d.grid_h) * c.grid_col + (c.W - 1) / d.grid_w + 1, d.n_cells);
    d.det_cells = c.det_rows * c.det_cols;
    d.cap = d.n_codes * std::max(c.grid_max, 1) + 8;
    d.cand_cap = d.n_cells * std::max(c.grid_max, 1) + 8;
    d.det_cap = d.det_cells;
    return d;
}

void fill_cfg(FeBookDev &B, const Cfg &c, const Dims &d) {
    std::memset(&B, 0, sizeof(B));
    B.grid_row = c.grid_row; B.grid_col = c.grid_col; B.grid_min = c.grid_min; B.grid_max = c.grid_max; B.n_codes = d.n_codes; B.n_cells = d.n_cells;
    B.grid_w = d.grid_w; B.grid_h = d.grid_h; B.det_rows = c.det_rows; B.det_cols = c.det_cols; B.det_cw = d.det_cw; B.det_ch = d.det_ch;
    B.thr_score = c.thr; B.q4 = c.q4; B.cap = d.cap; B.cand_cap = d.cand_cap; B.det_cap = d.det_cap;
    B.ransac = c.ransac; B.ransac_iters = static_cast<int>(std::ceil(std::log(1 - 0.99) / std::log(1 - 0.7 * 0.7))); B.ransac_thr = c.ransac_thr;
    for (int cam = 0; cam < 2; ++cam) { B.ransac_npu[cam] = 2.0 / (c.K[cam][0] + c.K[cam][1]); std::memcpy(B.R_p_c[cam], c.R[cam], sizeof(B.R_p_c[cam])); }
}

// the descriptor of frame `fr` for an arena at `base`
void desc_for(const Run &r, int fr, char *base, FeBookDev &B) {
    B = r.D;
    Carved K;
    fbc_carve(base, B, K, nullptr);
    B.prev = K.grid[fr & 1]; B.curr = K.grid[(fr & 1) ^ 1];
    B.gen = r.gen[fr];
}

// the frames of a named case
void make_frame(const Case &cs, const FrameSpec &s, const Dims &d, int fr, const std::vector<Feat> &flat, std::mt19937 &rng, Frame &f) {
    const Cfg &c = cs.c;
    auto U = [&](int lo, int hi) { return rnd_int(rng, lo, hi); };
    const int n = (int)flat.size();
    f.gen = (unsigned)((fr + 250) % 255) + 1;      // 251, 252, ...: the tag is not the frame number
    f.salt = rng();
    const int keep = s.keep < 0 || s.keep > n ? n : s.keep;
    f.t_out0.resize(n); f.t_out1.resize(n); f.t_und0.resize(n); f.t_und1.resize(n); f.t_status.resize(n);
    int kept_so_far = 0;
    for (int i = 0; i < n; ++i) {
        const bool kept = (long)(i + 1) * keep / n != (long)i * keep / n;
        f.t_status[i] = (uint8_t)(kept ? 3 : (s.lost >= 0 ? s.lost : (i & 1)));
        float x = flat[i].cam0.x, y = flat[i].cam0.y;
        if (s.place == 1) {
            const int kind = U(0, 19);
            x = (float)U(0, c.W - 2) + (float)U(0, 1023) / 1024.f; y = (float)U(0, c.H - 2) + (float)U(0, 1023) / 1024.f;
            if (kind == 0) x = (float)(c.W - 1);
            if (kind == 1) y = (float)(c.H - 1);
            if (kind == 2) { x = 0.f; y = 0.f; }
        } else if (s.place == 2) {
            x = 150.5f + (float)(i % 74); y = 60.25f + (float)((i / 74) % 59);
        } else if (s.place == 3) {
            const float px = (float)(c.grid_col * d.grid_w) + 0.25f, py = (float)(c.grid_row * d.grid_h) + 0.5f;     // first pixel of the partial column / row
            x = (float)U(0, c.W - 2) + 0.5f; y = (float)U(0, c.H - 2) + 0.25f;
            switch (i % 6) {
                case 0: x = (float)(c.W - 1); break;
                case 1: y = (float)(c.H - 1); break;
                case 2: if (px < (float)(c.W - 1)) x = px; break;
                case 3: if (py < (float)(c.H - 1)) y = py; break;
                case 4: x = (float)(c.W - 1); y = (float)(c.H - 1); break;
                default: break;
            }
        }
        f.t_out0[i] = mskf_point2f{x, y};
        f.t_out1[i] = mskf_point2f{x - 5.5f, y + 0.125f};
        f.t_und0[i] = mskf_point2f{x * 0.001f, y * 0.001f};
        f.t_und1[i] = mskf_point2f{x * 0.001f - 0.01f, y * 0.001f};
        if (s.und == 1) {
            const float zx = flat[i].und0.x * 0.1f * (float)U(0, 3) * s.flow_x, zy = flat[i].und0.y * 0.1f * (float)U(0, 3) * s.flow_y;
            const bool jump = s.wild_both > 0 && kept && kept_so_far >= s.wild_both;
            const float w0 = jump ? 0.3f : 0.f;
            const float w1 = jump ? 0.3f : (U(0, 99) < s.wild1_pct ? 0.03f : 0.f);
            f.t_und0[i] = mskf_point2f{flat[i].und0.x + s.flow_x + zx + 1e-5f * (float)U(-20, 20) + w0, flat[i].und0.y + s.flow_y + zy + 1e-5f * (float)U(-20, 20)};
            f.t_und1[i] = mskf_point2f{flat[i].und1.x + s.flow_x + zx + 1e-5f * (float)U(-20, 20) - w1 * 0.5f, flat[i].und1.y + s.flow_y + zy + 1e-5f * (float)U(-20, 20) + w1};
        } else if (s.und == 2) {
            for (int cam = 0; cam < 2; ++cam) {
                const double ang = 6.283185307179586 * (double)U(0, 9999) / 10000.0, mag = 0.02 + 0.07 * (double)U(0, 999) / 1000.0;
                const mskf_point2f p = cam == 0 ? flat[i].und0 : flat[i].und1;
                (cam == 0 ? f.t_und0[i] : f.t_und1[i]) = mskf_point2f{p.x + (float)(mag * std::cos(ang)), p.y + (float)(mag * std::sin(ang))};
            }
        }
        if (kept) ++kept_so_far;
        if (f.t_status[i] != 3) f.t_out1[i] = mskf_point2f{0, 0};
    }
    f.keys.assign(d.det_cells, 0ULL);
    for (int k = 0; k < d.det_cells; ++k) {
        if (U(0, 99) >= s.density) continue;
        const int cy = k / c.det_cols, cx = k - cy * c.det_cols;
        const int x0 = cx * d.det_cw, y0 = cy * d.det_ch;
        if (x0 >= c.W || y0 >= c.H) continue;
        const int ox = U(0, std::min(d.det_cw, c.W - x0) - 1), oy = U(0, std::min(d.det_ch, c.H - y0) - 1);
        const unsigned order = (unsigned)(oy * d.det_cw + ox);
        int score = U(0, 3) == 0 ? c.thr + U(-2, 2) : c.thr + 256 * U(1, 6);
        if (s.same_score) score = c.thr + 512;
        const unsigned gen = U(0, 99) < s.stale_pct ? ((f.gen + 7) % 255) + 1 : f.gen;
        f.keys[k] = ((u64)gen << 56) | ((u64)(unsigned)score << 32) | (0xFFFFFFFFu - order);
    }
}

// the seeded previous grid of frame 0, as ref_frame's map (flatten order = ascending code, insertion order inside a code)
void seed_grid(const Case &cs, const Dims &d, Grid &prev) {
    const Cfg &c = cs.c;
    for (int j = 0; j < cs.seed_n; ++j) {
        Feat ft;
        float x, y;
        if (cs.seed_mode == 1) {        // the middle of detector cell j
            const int cy = j / c.det_cols, cx = j % c.det_cols;
            x = std::min((float)(cx * d.det_cw) + 3.5f, (float)(c.W - 1)); y = std::min((float)(cy * d.det_ch) + 3.25f, (float)(c.H - 1));
        } else {
            const int cell = j % d.n_cells, k = j / d.n_cells, row = cell / c.grid_col, col = cell % c.grid_col;
            x = (float)(col * d.grid_w) + 1.5f + (float)((k * 5 + row) % (d.grid_w - 2)); y = (float)(row * d.grid_h) + 1.25f + (float)((k * 3 + col) % (d.grid_h - 2));
        }
        ft.id = (u64)j;
        ft.lifetime = cs.life_mode == 1 ? 5 : (cs.life_mode == 2 ? 2 + (j * 7) % 4 : 2 + (j * 13) % 9);
        ft.response = 0.f;
        ft.cam0 = mskf_point2f{x, y}; ft.cam1 = mskf_point2f{x - 5.5f, y + 0.125f};
        ft.und0 = mskf_point2f{(x - 188.f) * 0.002f, (y - 120.f) * 0.002f}; ft.und1 = mskf_point2f{(x - 193.5f) * 0.002f, (y - 120.f) * 0.002f};
        const int code = static_cast<int>(y / d.grid_h) * c.grid_col + static_cast<int>(x / d.grid_w);
        prev[code].push_back(ft);
    }
}

Run *run_case(int index) {
    Run *rp = new Run();
    Run &r = *rp;
    const Case &cs = cases()[index];
    r.cs = &cs;
    std::mt19937 rng(cs.random_trial >= 0 ? 777u + (unsigned)cs.random_trial : 4242u + 17u * (unsigned)index);
    auto U = [&](int lo, int hi) { return rnd_int(rng, lo, hi); };
    Cfg c = cs.c;
    int n_frames = (int)cs.frames.size();
    if (cs.random_trial >= 0) {
        gen_cfg(rng, cs.random_trial, c);
        c.grid_min = U(0, FB_MAXK); c.grid_max = U(c.grid_min, FB_MAXK);        // the limits book_alloc accepts
        n_frames = U(3, 8);
    }
    r.c = c;
    const Dims d = dims_of(c);
    fill_cfg(r.D, c, d);
    const size_t bytes = fbc_carve(nullptr, r.D, r.K, nullptr);
    std::vector<char> arena(bytes, (char)FILL);
    fbc_carve(arena.data(), r.D, r.K, &r.tab);
    r.scratch_bytes = 4 * fe_book_scratch_ints(d.cap, d.cand_cap, d.det_cap, d.n_codes, d.det_cells);
    FeBookState &st = *r.D.st;
    std::memset(&st, 0, sizeof(st));
    // reference-side state
    Grid prev, curr;
    Info info;
    u64 next_id = 0, ref_draws = 0;
    if (cs.seed_n > 0) {
        seed_grid(cs, d, prev);
        const FeGridArr &G = r.K.grid[0];
        int o = 0;
        for (const auto &it : prev)
            for (const auto &ft : it.second) {
                G.id[o] = ft.id; G.lifetime[o] = ft.lifetime; G.code[o] = it.first; G.response[o] = ft.response;
                G.cam0[o] = ft.cam0; G.cam1[o] = ft.cam1; G.und0[o] = ft.und0; G.und1[o] = ft.und1;
                ++o;
            }
        st.n_prev = st.n_curr = o;
        st.next_id = next_id = (u64)cs.seed_n;
    }
    r.init = arena;
    std::vector<int> scratch(r.scratch_bytes / 4);
    char msg[512];
    for (int fr = 0; fr < n_frames && r.error.empty(); ++fr) {
        Frame f;
        std::vector<Feat> flat;
        for (const auto &it : prev) for (const auto &pf : it.second) flat.push_back(pf);
        const int n = (int)flat.size();
        if (n != st.n_prev) { std::snprintf(msg, sizeof msg, "frame %d: n_prev %d vs %d", fr, st.n_prev, n); r.error = msg; break; }
        if (cs.random_trial >= 0) gen_frame(rng, c, fr, flat, f); else make_frame(cs, cs.frames[fr], d, fr, flat, rng, f);
        r.gen.push_back(f.gen);
        FeBookDev B;
        desc_for(r, fr, arena.data(), B);
        const FeGridArr &G = B.curr;
        // ---- inputs of fe_book1
        for (int i = 0; i < n; ++i) {
            const_cast<mskf_point2f *>(B.t_out0)[i] = f.t_out0[i]; const_cast<mskf_point2f *>(B.t_out1)[i] = f.t_out1[i];
            const_cast<mskf_point2f *>(B.t_und0)[i] = f.t_und0[i]; const_cast<mskf_point2f *>(B.t_und1)[i] = f.t_und1[i];
            const_cast<uint8_t *>(B.t_status)[i] = f.t_status[i];
        }
        for (int k = 0; k < d.det_cells; ++k) const_cast<unsigned long long *>(B.cell_keys)[k] = f.keys[k];
        r.snap.push_back(arena);
        const u64 draws_before = st.ransac_draws;
        FeBookScratch L;
        fe_book_scratch_init(L, scratch.data(), d.cap, d.cand_cap, d.det_cap, d.n_codes, d.det_cells);
        std::fill(scratch.begin(), scratch.end(), 0x5a5a5a5a);      // (nothing may depend on what the scratch held before)
        fe_book1(B, L);
        r.snap.push_back(arena);
        int ce[CE_WORDS] = {0};
        ce[CE_N_PREV] = n; ce[CE_N_TRACKED] = st.n_tracked; ce[CE_N_DET] = st.n_det; ce[CE_N_CAND] = st.n_cand;
        ce[CE_N_CELLS] = d.n_cells; ce[CE_GRID_MAX] = c.grid_max;
        if (c.ransac && st.after_matching > 0 && n > 0)
            for (int k = 0; k < st.after_matching; ++k) { ce[CE_IN0] += L.d[k] ? 1 : 0; ce[CE_IN1] += L.e[k] ? 1 : 0; }
        for (int code = 0; code < d.n_codes; ++code) ce[CE_MAX_TRACKED_CELL] = std::max(ce[CE_MAX_TRACKED_CELL], B.cell_count[code]);
        for (int code = 0; code < d.n_cells; ++code) {
            ce[CE_MAX_DET_CELL] = std::max(ce[CE_MAX_DET_CELL], L.cell[1][code]);
            ce[CE_CELLS_WITH_CAND] += B.cand_cnt[code] > 0 ? 1 : 0;
        }
        ce[CE_SCORE_LO] = st.n_det ? 0x7fffffff : 0;
        for (int q = 0; q < st.n_det; ++q) { ce[CE_SCORE_LO] = std::min(ce[CE_SCORE_LO], B.det_score[q]); ce[CE_SCORE_HI] = std::max(ce[CE_SCORE_HI], B.det_score[q]); }
        for (int k = 0; k < st.n_tracked; ++k) ce[CE_MAX_CODE] = std::max(ce[CE_MAX_CODE], B.tracked.code[k]);
        for (int k = 0; k < d.det_cells; ++k) ce[CE_KEYS] += (unsigned)(f.keys[k] >> 56) == f.gen ? 1 : 0;
        // ---- the stereo outcome of the candidates
        const int cand_mode = cs.random_trial >= 0 ? 0 : cs.frames[fr].cand;
        g_cand_mode = cand_mode; g_pass.clear();
        g_cand_status_hook = cand_mode ? cand_hook : nullptr;
        if (cand_mode == 3)
            for (int code = 0; code < d.n_cells; ++code)
                if (B.cand_cnt[code] > 0) g_pass.insert(bits_of(B.cand_pt[B.cand_off[code] + B.cand_cnt[code] - 1]));
        // ---- reference
        std::vector<mskf_point2f> ref_cand; std::vector<int> ref_cand_index;
        ref_frame(c, f, prev, curr, info, next_id, ref_draws, ref_cand, ref_cand_index);
        if (st.n_cand != (int)ref_cand.size()) { std::snprintf(msg, sizeof msg, "frame %d: %d candidates vs %d", fr, st.n_cand, (int)ref_cand.size()); r.error = msg; break; }
        for (int i = 0; i < st.n_cand; ++i) {
            if (!same_pt(B.cand_pt[i], ref_cand[i]) || B.cand_index[i] != ref_cand_index[i]) { std::snprintf(msg, sizeof msg, "frame %d: candidate %d differs", fr, i); r.error = msg; break; }
            mskf_point2f o1, u0, u1; uint8_t s;
            cand_result(B.cand_pt[i], f.salt, o1, u0, u1, s);
            const_cast<mskf_point2f *>(B.c_out0)[i] = B.cand_pt[i]; const_cast<mskf_point2f *>(B.c_out1)[i] = o1;
            const_cast<mskf_point2f *>(B.c_und0)[i] = u0; const_cast<mskf_point2f *>(B.c_und1)[i] = u1; const_cast<uint8_t *>(B.c_status)[i] = s;
        }
        if (!r.error.empty()) break;
        r.snap.push_back(arena);
        std::fill(scratch.begin(), scratch.end(), 0x3c3c3c3c);
        fe_book2(B, L);
        r.snap.push_back(arena);
        g_cand_status_hook = nullptr;
        // ---- compare the published grid, the id counter and the tracking info
        std::vector<Feat> want; std::vector<int> want_code;
        for (const auto &it : curr)
            for (const auto &ft : it.second) { want.push_back(ft); want_code.push_back(it.first); }
        if (st.n_curr != (int)want.size() || B.x_info[0] != st.n_curr) { std::snprintf(msg, sizeof msg, "frame %d: %d features vs %d", fr, st.n_curr, (int)want.size()); r.error = msg; break; }
        for (int i = 0; i < st.n_curr; ++i) {
            const bool ok = G.id[i] == want[i].id && G.lifetime[i] == want[i].lifetime && G.code[i] == want_code[i] &&
                            std::memcmp(&G.response[i], &want[i].response, 4) == 0 && same_pt(G.cam0[i], want[i].cam0) && same_pt(G.cam1[i], want[i].cam1) &&
                            same_pt(G.und0[i], want[i].und0) && same_pt(G.und1[i], want[i].und1) &&
                            B.x_id[i] == want[i].id && B.x_lifetime[i] == want[i].lifetime && same_pt(B.x_cam0[i], want[i].cam0) && same_pt(B.x_cam1[i], want[i].cam1) &&
                            same_pt(B.x_und0[i], want[i].und0) && same_pt(B.x_und1[i], want[i].und1);
            if (!ok) {
                std::snprintf(msg, sizeof msg, "frame %d: feature %d differs (id %llu vs %llu, life %d vs %d, code %d vs %d)", fr, i, G.id[i], want[i].id,
                              G.lifetime[i], want[i].lifetime, G.code[i], want_code[i]);
                r.error = msg;
                break;
            }
        }
        if (!r.error.empty()) break;
        if (st.ransac_draws != ref_draws) { std::snprintf(msg, sizeof msg, "frame %d: RANSAC draw counter %llu vs %llu", fr, st.ransac_draws, ref_draws); r.error = msg; break; }
        if (st.next_id != next_id) { std::snprintf(msg, sizeof msg, "frame %d: next id %llu vs %llu", fr, st.next_id, next_id); r.error = msg; break; }
        if (st.before_tracking != info.before || st.after_tracking != info.after_tracking || st.after_matching != info.after_matching ||
            st.after_ransac != info.after_ransac) { std::snprintf(msg, sizeof msg, "frame %d: tracking info", fr); r.error = msg; break; }
        ce[CE_N_NEW] = st.n_new; ce[CE_N_CURR] = st.n_curr; ce[CE_DRAWS] = (int)(st.ransac_draws - draws_before); ce[CE_OVERFLOW] = st.overflow;
        ce[CE_BEFORE] = st.before_tracking; ce[CE_AFTER_TRACKING] = st.after_tracking; ce[CE_AFTER_MATCHING] = st.after_matching; ce[CE_AFTER_RANSAC] = st.after_ransac;
        for (const auto &it : curr) ce[CE_MAX_CURR_CELL] = std::max(ce[CE_MAX_CURR_CELL], (int)it.second.size());
        // NaNs among the doubles and floats the kernels wrote (their bit patterns are the platform's)
        for (const Arr &a : r.tab) {
            if (std::strcmp(a.name, "rs_scalar") == 0 || std::strcmp(a.name, "rs_pair") == 0)
                for (size_t k = 0; k < a.bytes / 8; ++k) { double v; std::memcpy(&v, arena.data() + a.off + 8 * k, 8); ce[CE_NAN_WORDS] += std::isnan(v) ? 1 : 0; }
        }
        r.census.insert(r.census.end(), ce, ce + CE_WORDS);
        prev = curr;
    }
    g_cand_status_hook = nullptr;
    return rp;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C interface (ctypes)
extern "C" {
int fbc_host_order(void) {
#ifdef FB_HOST_ORDER
    return FB_HOST_ORDER;
#else
    return 0;
#endif
}
int fbc_n_cases(void) { return (int)cases().size(); }
const char *fbc_case_name(int i) { return cases()[i].name.c_str(); }
const char *fbc_case_set(int i) { return cases()[i].set.c_str(); }
int fbc_census_words(void) { return CE_WORDS; }
const char *fbc_census_names(void) {
    return "n_prev n_tracked n_det n_cand n_new n_curr draws overflow before after_tracking after_matching after_ransac max_tracked_cell "
           "max_curr_cell max_code n_cells cells_with_cand score_lo score_hi in0 in1 max_det_cell nan_words keys grid_max";
}
void *fbc_run(int i) { return i >= 0 && i < (int)cases().size() ? run_case(i) : nullptr; }
void fbc_free(void *h) { delete (Run *)h; }
const char *fbc_error(void *h) { return ((Run *)h)->error.c_str(); }
int fbc_n_frames(void *h) { return (int)((Run *)h)->snap.size() / 4; }
size_t fbc_desc_size(void) { return sizeof(FeBookDev); }
size_t fbc_arena_size(void *h) { return ((Run *)h)->K.size; }
size_t fbc_scratch_bytes(void *h) { return ((Run *)h)->scratch_bytes; }
const void *fbc_initial(void *h) { return ((Run *)h)->init.data(); }
const void *fbc_snapshot(void *h, int frame, int which) { return ((Run *)h)->snap[(size_t)4 * frame + which].data(); }
const int *fbc_census(void *h, int frame) { return ((Run *)h)->census.data() + (size_t)CE_WORDS * frame; }
// which = 0: the inputs of fe_book1, 1: the inputs of fe_book2; byte range of the arena
void fbc_input_range(void *h, int which, size_t *lo, size_t *hi) {
    const Carved &K = ((Run *)h)->K;
    *lo = which ? K.c_lo : K.in_lo; *hi = which ? K.c_hi : K.in_hi;
}
int fbc_n_arrays(void *h) { return (int)((Run *)h)->tab.size(); }
const char *fbc_array(void *h, int k, size_t *off, size_t *bytes, size_t *elem) {
    const Arr &a = ((Run *)h)->tab[k];
    *off = a.off; *bytes = a.bytes; *elem = a.elem;
    return a.name;
}
// the descriptor of frame `frame` for an arena at address `base` (host or device)
void fbc_desc(void *h, int frame, unsigned long long base, void *out) {
    FeBookDev B;
    desc_for(*(Run *)h, frame, (char *)(uintptr_t)base, B);
    std::memcpy(out, &B, sizeof(B));
}
// Self-check of a filled descriptor against the arena [base, base + size): every pointer and its extent inside, the
// capacities those of book_alloc, the scratch within `lds_budget`, n_prev (of the host arena at that frame) <= cap.
// Returns 0, or the number of the first failed check (and says which in `why`).
int fbc_check_desc(void *h, int frame, const void *desc, unsigned long long base, size_t size, size_t lds_budget, char *why, size_t why_len) {
    const Run &r = *(Run *)h;
    FeBookDev B;
    std::memcpy(&B, desc, sizeof(B));
    const Dims d = dims_of(r.c);
    int no = 0;
    auto fail = [&](const char *what) { std::snprintf(why, why_len, "%s", what); return no; };
    ++no; if (B.cap != d.cap || B.cand_cap != d.cand_cap || B.det_cap != d.det_cap || B.n_codes != d.n_codes || B.n_cells != d.n_cells) return fail("capacities");
    ++no; if (B.grid_h != d.grid_h || B.grid_w != d.grid_w || B.det_ch != d.det_ch || B.det_cw != d.det_cw || B.det_rows * B.det_cols != d.det_cells) return fail("geometry");
    ++no; if (B.grid_min < 0 || B.grid_min > B.grid_max || B.grid_max > FB_MAXK) return fail("grid_min / grid_max");
    ++no; if (B.ransac_iters < 0 || B.ransac_iters > 8) return fail("ransac_iters");
    ++no; if (4 * fe_book_scratch_ints(B.cap, B.cand_cap, B.det_cap, B.n_codes, B.det_rows * B.det_cols) != r.scratch_bytes || r.scratch_bytes > lds_budget) return fail("scratch size");
    const size_t cap = (size_t)B.cap, cand_cap = (size_t)B.cand_cap, det_cap = (size_t)B.det_cap;
    std::vector<std::pair<uintptr_t, uintptr_t>> ext;
    auto in = [&](const void *p, size_t bytes, size_t align) {
        const uintptr_t a = (uintptr_t)p;
        if (!(a >= base && a % align == 0 && bytes <= size && a - base <= size - bytes)) return false;
        ext.push_back(std::make_pair(a, a + bytes));
        return true;
    };
    auto grid = [&](const FeGridArr &G) {
        return in(G.id, 8 * cap, 8) && in(G.lifetime, 4 * cap, 4) && in(G.code, 4 * cap, 4) && in(G.response, 4 * cap, 4) && in(G.cam0, 8 * cap, 4) &&
               in(G.cam1, 8 * cap, 4) && in(G.und0, 8 * cap, 4) && in(G.und1, 8 * cap, 4);
    };
    ++no; if (!in(B.st, sizeof(FeBookState), 8)) return fail("state pointer");
    ++no; if (!grid(B.prev) || !grid(B.curr) || !grid(B.tracked)) return fail("grid pointers");
    ++no; if (!in(B.det_pt, 8 * det_cap, 4) || !in(B.det_score, 4 * det_cap, 4) || !in(B.cell_keys, 8 * det_cap, 8)) return fail("detection pointers");
    ++no; if (!in(B.cand_pt, 8 * cand_cap, 4) || !in(B.cand_index, 4 * cand_cap, 4) || !in(B.cand_score, 4 * cand_cap, 4) ||
              !in(B.cand_off, 4 * ((size_t)B.n_cells + 1), 4) || !in(B.cand_cnt, 4 * ((size_t)B.n_cells + 1), 4) || !in(B.cell_count, 4 * ((size_t)B.n_codes + 1), 4))
        return fail("candidate pointers");
    ++no; if (!in(B.t_out0, 8 * cap, 4) || !in(B.t_out1, 8 * cap, 4) || !in(B.t_und0, 8 * cap, 4) || !in(B.t_und1, 8 * cap, 4) || !in(B.t_status, cap, 1)) return fail("track result pointers");
    ++no; if (!in(B.c_out0, 8 * cand_cap, 4) || !in(B.c_out1, 8 * cand_cap, 4) || !in(B.c_und0, 8 * cand_cap, 4) || !in(B.c_und1, 8 * cand_cap, 4) || !in(B.c_status, cand_cap, 1))
        return fail("candidate result pointers");
    ++no; if (!in(B.rs_pair, 8 * 4 * cap, 8) || !in(B.rs_pt, 4 * 4 * cap, 4) || !in(B.rs_scalar, 8 * 48, 8)) return fail("RANSAC scratch pointers");
    ++no; if (!in(B.x_info, 4 * FX_WORDS, 4) || !in(B.x_id, 8 * cap, 8) || !in(B.x_lifetime, 4 * cap, 4) || !in(B.x_cam0, 8 * cap, 4) || !in(B.x_cam1, 8 * cap, 4) ||
              !in(B.x_und0, 8 * cap, 4) || !in(B.x_und1, 8 * cap, 4)) return fail("export pointers");
    std::sort(ext.begin(), ext.end());
    ++no; for (size_t k = 1; k < ext.size(); ++k) if (ext[k].first < ext[k - 1].second) return fail("two arrays overlap");
    ++no; if (B.prev.id == B.curr.id || B.gen != r.gen[frame] || B.gen < 1 || B.gen > 255) return fail("per-frame part");
    FeBookState st;
    std::memcpy(&st, r.snap[(size_t)4 * frame].data() + r.tab[0].off, sizeof(st));
    ++no; if (st.n_prev < 0 || st.n_prev > B.cap) return fail("n_prev > cap");
    return 0;
}
}
