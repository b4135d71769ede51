// fe_book_test.cpp — CPU check of the front-end's device bookkeeping (msckf_stereo_c_amd/csrc/hip/fe_book.h).
//
// fe_book.h is written so that the SAME source runs on the host (phases of independent items, no atomics, no cross-lane
// operations): here fe_book1 / fe_book2 are executed on random frames — random previous grids, random track results
// (including points on the image border and in the partial grid rows / columns of quirk Q7), random detector keys with
// many score ties and stale generations, random outcomes of the candidates' stereo match — and compared, frame after
// frame with the state carried over, with a plain restatement of the reference's own flow built on std::map and
// std::stable_sort (image_processor.cpp:416-513 trackFeatures tail, :622-756 addNewFeatures, :758-768 pruneGridFeatures;
// the same structure as oracle/o_frontend.cpp).  Everything is integer / float-exact, so the comparison is bitwise.
//
// build: g++ -O2 -std=c++17 -I<repo> tests/cpp/fe_book_test.cpp -o fe_book_test      run: ./fe_book_test [trials]
#include "fe_book_scenarios.h"

// ---------------------------------------------------------------------------------------------- device-logic side
struct HostGrid {
    std::vector<u64> id; std::vector<int> lifetime, code; std::vector<float> response; std::vector<mskf_point2f> cam0, cam1, und0, und1;
    void resize(int n) { id.resize(n); lifetime.resize(n); code.resize(n); response.resize(n); cam0.resize(n); cam1.resize(n); und0.resize(n); und1.resize(n); }
    FeGridArr arr() { return FeGridArr{id.data(), lifetime.data(), code.data(), response.data(), cam0.data(), cam1.data(), und0.data(), und1.data()}; }
};

static bool same_pt(mskf_point2f a, mskf_point2f b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main(int argc, char **argv) {
    const int trials = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937 rng(12345);
    auto U = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    long frames_checked = 0, feats_checked = 0, pruned_cells = 0, cand_total = 0, ransac_rejected = 0, draws_total = 0;
    for (int trial = 0; trial < trials; ++trial) {
        Cfg c;
        gen_cfg(rng, trial, c);
        const int grid_h = c.H / c.grid_row, grid_w = c.W / c.grid_col;
        const int det_ch = (c.H + c.det_rows - 1) / c.det_rows, det_cw = (c.W + c.det_cols - 1) / c.det_cols;
        const int n_cells = c.grid_row * c.grid_col;
        const int n_codes = std::max(((c.H - 1) / grid_h) * c.grid_col + (c.W - 1) / grid_w + 1, n_cells);
        const int det_cells = c.det_rows * c.det_cols;
        const int cap = n_codes * c.grid_max + 8, cand_cap = n_cells * c.grid_max + 8, det_cap = det_cells;
        // device-side state
        HostGrid g[3];
        for (auto &x : g) x.resize(cap);
        FeBookState st;
        std::memset(&st, 0, sizeof(st));
        std::vector<int> scratch(fe_book_scratch_ints(cap, cand_cap, det_cap, n_codes, det_cells));
        std::vector<mskf_point2f> det_pt(det_cap), cand_pt(cand_cap), c_out0(cand_cap), c_out1(cand_cap), c_und0(cand_cap), c_und1(cand_cap);
        std::vector<int> det_score(det_cap), cand_index(cand_cap), cand_score(cand_cap), cand_off(n_cells + 1), cand_cnt(n_cells + 1), cell_count(n_codes + 1);
        std::vector<uint8_t> c_status(cand_cap);
        std::vector<int> x_info(16); std::vector<u64> x_id(cap); std::vector<int> x_life(cap);
        std::vector<mskf_point2f> x_c0(cap), x_c1(cap), x_u0(cap), x_u1(cap);
        int ip = 0;     // index of the "prev" grid among g[0], g[1]; g[2] is the tracked list
        // reference-side state
        Grid prev, curr;
        Info info;
        u64 next_id = 0, ref_draws = 0;
        std::vector<double> rs_pair(4 * (size_t)cap), rs_scalar(48);
        std::vector<float> rs_pt(4 * (size_t)cap);
        const int n_frames = U(3, 8);
        for (int fr = 0; fr < n_frames; ++fr) {
            Frame f;
            std::vector<Feat> flat;
            for (const auto &it : prev) for (const auto &pf : it.second) flat.push_back(pf);
            const int n = (int)flat.size();
            if (n != st.n_prev) { std::printf("FAIL trial %d frame %d: n_prev %d vs %d\n", trial, fr, st.n_prev, n); return 1; }
            gen_frame(rng, c, fr, flat, f);
            // ---- reference
            std::vector<mskf_point2f> ref_cand; std::vector<int> ref_cand_index;
            ref_frame(c, f, prev, curr, info, next_id, ref_draws, ref_cand, ref_cand_index);
            // ---- device logic
            FeBookDev B;
            std::memset(&B, 0, sizeof(B));
            B.grid_row = c.grid_row; B.grid_col = c.grid_col; B.grid_min = c.grid_min; B.grid_max = c.grid_max; B.n_codes = n_codes; B.n_cells = n_cells;
            B.grid_w = grid_w; B.grid_h = grid_h; B.det_rows = c.det_rows; B.det_cols = c.det_cols; B.det_cw = det_cw; B.det_ch = det_ch;
            B.thr_score = c.thr; B.q4 = c.q4; B.cap = cap; B.cand_cap = cand_cap; B.det_cap = det_cap; B.gen = f.gen; B.st = &st;
            B.prev = g[ip].arr(); B.curr = g[ip ^ 1].arr(); B.tracked = g[2].arr();
            B.t_out0 = f.t_out0.data(); B.t_out1 = f.t_out1.data(); B.t_und0 = f.t_und0.data(); B.t_und1 = f.t_und1.data(); B.t_status = f.t_status.data();
            B.cell_keys = f.keys.data(); B.det_pt = det_pt.data(); B.det_score = det_score.data();
            B.cand_pt = cand_pt.data(); B.cand_index = cand_index.data(); B.cand_score = cand_score.data(); B.cand_off = cand_off.data(); B.cand_cnt = cand_cnt.data();
            B.c_out0 = c_out0.data(); B.c_out1 = c_out1.data(); B.c_und0 = c_und0.data(); B.c_und1 = c_und1.data(); B.c_status = c_status.data();
            B.cell_count = cell_count.data();
            B.ransac = c.ransac; B.ransac_iters = 7; B.ransac_thr = c.ransac_thr;
            for (int cam = 0; cam < 2; ++cam) { B.ransac_npu[cam] = 2.0 / (c.K[cam][0] + c.K[cam][1]); std::memcpy(B.R_p_c[cam], c.R[cam], sizeof(B.R_p_c[cam])); }
            B.rs_pair = rs_pair.data(); B.rs_pt = rs_pt.data(); B.rs_scalar = rs_scalar.data();
            B.x_info = x_info.data(); B.x_id = x_id.data(); B.x_lifetime = x_life.data(); B.x_cam0 = x_c0.data(); B.x_cam1 = x_c1.data(); B.x_und0 = x_u0.data(); B.x_und1 = x_u1.data();
            FeBookScratch L;
            fe_book_scratch_init(L, scratch.data(), cap, cand_cap, det_cap, n_codes, det_cells);
            std::fill(scratch.begin(), scratch.end(), 0x5a5a5a5a);      // (nothing may depend on what the scratch held before)
            fe_book1(B, L);
            // candidates: the reference's list restricted to the cells with a vacancy, same order, same positions
            if (st.n_cand != (int)ref_cand.size()) { std::printf("FAIL trial %d frame %d: %d candidates vs %d\n", trial, fr, st.n_cand, (int)ref_cand.size()); return 1; }
            for (int i = 0; i < st.n_cand; ++i) {
                if (!same_pt(cand_pt[i], ref_cand[i]) || cand_index[i] != ref_cand_index[i]) { std::printf("FAIL trial %d frame %d: candidate %d differs: pt (%g,%g) vs (%g,%g), index %d vs %d, score %d\n", trial, fr, i, cand_pt[i].x, cand_pt[i].y, ref_cand[i].x, ref_cand[i].y, cand_index[i], ref_cand_index[i], cand_score[i]); return 1; }
                mskf_point2f o1, u0, u1; uint8_t s;
                cand_result(cand_pt[i], f.salt, o1, u0, u1, s);
                c_out0[i] = cand_pt[i]; c_out1[i] = o1; c_und0[i] = u0; c_und1[i] = u1; c_status[i] = s;
            }
            cand_total += st.n_cand;
            std::fill(scratch.begin(), scratch.end(), 0x3c3c3c3c);
            fe_book2(B, L);
            // ---- compare the published grid, the id counter and the tracking info
            std::vector<Feat> want; std::vector<int> want_code;
            for (const auto &it : curr) {
                for (const auto &ft : it.second) { want.push_back(ft); want_code.push_back(it.first); }
            }
            if (st.overflow) { std::printf("FAIL trial %d frame %d: overflow flag\n", trial, fr); return 1; }
            if (st.n_curr != (int)want.size() || x_info[0] != st.n_curr) { std::printf("FAIL trial %d frame %d: %d features vs %d\n", trial, fr, st.n_curr, (int)want.size()); return 1; }
            for (int i = 0; i < st.n_curr; ++i) {
                const HostGrid &G = g[ip ^ 1];
                const bool ok = G.id[i] == want[i].id && G.lifetime[i] == want[i].lifetime && G.code[i] == want_code[i] &&
                                std::memcmp(&G.response[i], &want[i].response, 4) == 0 && same_pt(G.cam0[i], want[i].cam0) && same_pt(G.cam1[i], want[i].cam1) &&
                                same_pt(G.und0[i], want[i].und0) && same_pt(G.und1[i], want[i].und1) &&
                                x_id[i] == want[i].id && x_life[i] == want[i].lifetime && same_pt(x_c0[i], want[i].cam0) && same_pt(x_c1[i], want[i].cam1) &&
                                same_pt(x_u0[i], want[i].und0) && same_pt(x_u1[i], want[i].und1);
                if (!ok) {
                    std::printf("FAIL trial %d frame %d: feature %d differs (id %llu vs %llu, life %d vs %d, code %d vs %d)\n", trial, fr, i, G.id[i], want[i].id,
                                G.lifetime[i], want[i].lifetime, G.code[i], want_code[i]);
                    return 1;
                }
            }
            if (st.ransac_draws != ref_draws) { std::printf("FAIL trial %d frame %d: RANSAC draw counter %llu vs %llu\n", trial, fr, st.ransac_draws, ref_draws); return 1; }
            ransac_rejected += info.after_matching - info.after_ransac;
            if (fr == n_frames - 1) draws_total += (long)ref_draws;
            if (st.next_id != next_id) { std::printf("FAIL trial %d frame %d: next id %llu vs %llu\n", trial, fr, st.next_id, next_id); return 1; }
            if (st.before_tracking != info.before || st.after_tracking != info.after_tracking || st.after_matching != info.after_matching ||
                st.after_ransac != info.after_ransac) { std::printf("FAIL trial %d frame %d: tracking info\n", trial, fr); return 1; }
            for (const auto &it : curr) pruned_cells += (int)it.second.size() == c.grid_max ? 1 : 0;
            feats_checked += st.n_curr; ++frames_checked;
            prev = curr;
            ip ^= 1;
        }
    }
    std::printf("fe_book: %ld frames, %ld features, %ld candidates, %ld full cells, %ld RANSAC rejections (%ld numbers drawn, counter checked every frame): device logic == reference flow\n",
                frames_checked, feats_checked, cand_total, pruned_cells, ransac_rejected, draws_total);
    return 0;
}
