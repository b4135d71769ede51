// batch_runner.cpp — see batch_runner.h.
#include "batch_runner.h"
#include "host_prof.h"
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstring>

namespace cg {

ForkJoin::ForkJoin(int n_threads) : nt_(n_threads) {
    for (int i = 1; i < nt_; ++i) th_.emplace_back([this, i]() { worker(i); });
}
ForkJoin::~ForkJoin() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
}
void ForkJoin::worker(int) {
    unsigned long long seen = 0;
    for (;;) {
        const std::function<void(int)> *fn;
        int n;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&]() { return gen_ != seen; });
            seen = gen_;
            if (stop_) return;
            fn = fn_; n = n_;
            hostprof::enabled() = prof_on_;
        }
        for (int i = next_.fetch_add(1); i < n; i = next_.fetch_add(1)) (*fn)(i);
        done_.fetch_add(1);
    }
}
void ForkJoin::run(int n, const std::function<void(int)> &fn) {
    if (nt_ <= 1 || n <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    next_.store(0); done_.store(0);
    { std::lock_guard<std::mutex> lk(mu_); fn_ = &fn; n_ = n; prof_on_ = hostprof::enabled(); ++gen_; }
    cv_.notify_all();
    for (int i = next_.fetch_add(1); i < n; i = next_.fetch_add(1)) fn(i);
    while (done_.load() < nt_ - 1) std::this_thread::yield();
}

BatchGroup::BatchGroup(int device, int n, const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf, int host_threads, int ekf_host_threads) {
    // per-stream host phases of a group are independent: optional helper threads for the front-end / filter stages
    const int ht_fe = std::max(1, host_threads), ht_ekf = std::max(1, ekf_host_threads > 0 ? ekf_host_threads : host_threads);
    if (ht_fe > 1) { pool_.reset(new ForkJoin(ht_fe)); par_fe_ = [this](int cnt, const std::function<void(int)> &fn) { pool_->run(cnt, fn); }; }
    if (ht_ekf > 1) { pool_ekf_.reset(new ForkJoin(ht_ekf)); par_ekf_ = [this](int cnt, const std::function<void(int)> &fn) { pool_ekf_->run(cnt, fn); }; }
    int rc = mskf_ctx_create(device, &ctx_);
    if (rc == MSKF_OK) rc = mskf_ctx_create_prio(device, 1, &ekf_ctx_);     // the filter is the serial chain of a frame: its queue is dispatched first
    if (rc != MSKF_OK) { error_ = mskf_last_error(); return; }
    home_fe_ = ctx_; home_ekf_ = ekf_ctx_;
    for (int i = 0; i < n; ++i) {
        systems_.emplace_back(new System(calib, fe, ekf, ctx_, device));
        if (!systems_.back()->ok()) { error_ = std::string("stream setup failed: ") + mskf_last_error(); return; }
        systems_.back()->copy_draw_buffers = false;
        systems_.back()->imgproc_ptr_->setCompactTail(true);      // the Q1 tail of the message as a count (image_processor.h)
        streams_.push_back(systems_.back()->stream());
        ips_.push_back(systems_.back()->imgproc_ptr_.get()); vios_.push_back(systems_.back()->msckfvio_ptr().get());
        // the filter half of every stream runs on its own context (own HIP stream): no device data is shared
        if (mskf_stream_set_ekf_ctx(streams_.back(), ekf_ctx_) != MSKF_OK) { error_ = mskf_last_error(); return; }
    }
    p0_.resize(n); p1_.resize(n); t_.resize(n);
    seq.resize(n);
    ok_ = true;
}

BatchGroup::~BatchGroup() {
    rebind_home();
    if (ekf_tail_) mskf_point_destroy(ekf_tail_);
    systems_.clear();
    if (ekf_ctx_) mskf_ctx_destroy(ekf_ctx_);
    if (ctx_) mskf_ctx_destroy(ctx_);
}

static std::shared_ptr<Imu> imu_msg(const mskf_imu_sample &s) {
    std::shared_ptr<Imu> m(new Imu);
    m->time_stamp = s.time_stamp;
    m->angular_velocity = Vector3(s.angular_velocity[0], s.angular_velocity[1], s.angular_velocity[2]);
    m->linear_acceleration = Vector3(s.linear_acceleration[0], s.linear_acceleration[1], s.linear_acceleration[2]);
    return m;
}

void BatchGroup::imu(int i, const mskf_imu_sample &s) { systems_[i]->imu_callback(imu_msg(s)); }

// Front-end of one frame of every stream (System::stereo_callback): ImageProcessor::runFrame over the group, on the context
// and into the accumulator of whoever runs the stage; the Systems then see the published messages.
int BatchGroup::step_fe(const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, const double *t, bool is_draw) {
    const int n = size();
    if (!ok_ || n == 0) return MSKF_ERR_INVALID;
    std::string what;
    const int rc = ImageProcessor::runFrame(ctx_, n, ips_.data(), streams_.data(), cam0, cam1, on_device, t, is_draw, fe_scratch_, par_fe_,
                                            acc_fe_ ? acc_fe_ : phase_s, what);
    if (rc != MSKF_OK) { error_ = what + ": " + mskf_last_error(); return rc; }
    for (int i = 0; i < n; ++i) systems_[i]->set_feature_msg(ips_[i]->feature_msg_ptr_);
    return MSKF_OK;
}

// Filter of one frame of every stream (System::backend_callback -> MsckfVio::featureCallback): MsckfVio::runFrame over the
// group, on the messages of the hand-off (a pipelined run) or of the Systems, each with its zero-tail hint.
int BatchGroup::step_ekf(const FrameBatch *fb) {
    const int n = size();
    std::vector<CameraMeasurementConstPtr> msgs(n);
    for (int i = 0; i < n; ++i) {
        if (fb) { msgs[i] = fb->msg[i]; vios_[i]->setZeroTailHint(msgs[i].get(), fb->tail_start[i], fb->total[i]); }
        else {
            msgs[i] = systems_[i]->feature_msg();
            vios_[i]->setZeroTailHint(msgs[i].get(), ips_[i]->zeroTailStart(), ips_[i]->messageSize());
        }
    }
    std::string what;
    const int rc = MsckfVio::runFrame(ekf_ctx_, n, vios_.data(), streams_.data(), msgs.data(), ekf_scratch_, par_ekf_, acc_ekf_ ? acc_ekf_ : phase_s, what);
    if (rc != MSKF_OK) error_ = what + ": " + mskf_last_error();
    return rc;
}

int BatchGroup::step(const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, const double *t, bool is_draw) {
    const int rc = step_fe(cam0, cam1, on_device, t, is_draw);
    return rc != MSKF_OK ? rc : step_ekf(nullptr);
}

static double ns_to_sec(long long ns) {   // apps/run_euroc_single_thread.cpp:164-166,192 (Q9)
    const long long sec = ns / 1000000000LL, nsec = ns % 1000000000LL;
    const double stamp_ns = (double)(int)sec * 1e9 + (double)(int)nsec;
    return stamp_ns * 1e-9;
}

// do { feed IMU } while (t_imu <= t_img)  (apps/run_euroc_single_thread.cpp:209-238, Q10) for frame k of every stream
int BatchGroup::feed_imu(int k, bool to_fe, bool to_ekf) {
    const int n = size();
    for (int i = 0; i < n; ++i) {
        StreamSequence &q = seq[i];
        if (!q.cam0_base || !q.imu) { error_ = "no sequence attached"; return MSKF_ERR_INVALID; }
        const double t_img = ns_to_sec(q.t0_ns + (long long)k * q.frame_dt_ns);
        int &cur = to_fe ? q.imu_cursor : q.imu_cursor_ekf;
        double t_imu = 0.0;
        do {
            if (cur >= q.n_imu) { error_ = "IMU sequence exhausted"; return MSKF_ERR_CAPACITY; }
            const mskf_imu_sample &s = q.imu[cur++];
            const std::shared_ptr<Imu> m = imu_msg(s);
            if (to_fe) systems_[i]->imgproc_ptr_->imuCallback(m);      // System::imu_callback, system.cpp:45-48
            if (to_ekf) systems_[i]->msckfvio_ptr()->imuCallback(m);
            t_imu = s.time_stamp;
        } while (t_imu <= t_img);
        if (to_fe && to_ekf) q.imu_cursor_ekf = q.imu_cursor;
        if (to_fe) {
            const int key = k < q.n_static ? k : q.n_static + (k - q.n_static) % q.n_loop;
            p0_[i] = q.cam0_base + (size_t)key * q.frame_bytes;
            p1_[i] = q.cam1_base + (size_t)key * q.frame_bytes;
            t_[i] = t_img;
        }
    }
    return MSKF_OK;
}

int BatchGroup::run(int first, int n_frames) {
    for (int k = first; k < first + n_frames; ++k) {
        auto t_imu0 = std::chrono::steady_clock::now();
        int rc = feed_imu(k, true, true);
        if (rc != MSKF_OK) return rc;
        phase_s[PH_IMU] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_imu0).count();
        rc = step(p0_.data(), p1_.data(), seq[0].on_device, t_.data(), false);
        if (rc != MSKF_OK) return rc;
    }
    return MSKF_OK;
}

// hand-off = a snapshot of every stream's message (live + stale entries + the first tail record); `fb` is recycled when given
void BatchGroup::fill_handoff(int k, std::unique_ptr<FrameBatch> &fb) {
    const int n = size();
    if (!fb) fb.reset(new FrameBatch);
    fb->frame = k;
    fb->msg.resize(n); fb->tail_start.resize(n); fb->total.resize(n);
    for (int i = 0; i < n; ++i) {
        const ImageProcessor &ip = *systems_[i]->imgproc_ptr_;
        const CameraMeasurement &live = *ip.feature_msg_ptr_;
        const size_t total = ip.messageSize(), start = ip.zeroTailStart();
        const size_t keep = std::min(live.features.size(), start + 1);
        if (!fb->msg[i] || fb->msg[i].use_count() > 1) fb->msg[i].reset(new CameraMeasurement);
        fb->msg[i]->time_stamp = live.time_stamp;
        fb->msg[i]->features.assign(live.features.begin(), live.features.begin() + keep);
        fb->tail_start[i] = start; fb->total[i] = total;
    }
}

void BatchGroup::snapshot_fe_mark() {
    std::vector<ImageProcessor::FeatureIDType> ids;
    systems_[0]->imgproc_ptr_->dumpCurrent(ids, mark_dump.life, mark_dump.c0, mark_dump.c1);
    mark_dump.ids.assign(ids.begin(), ids.end());
    mark_dump.fe_valid = true;
}

void BatchGroup::snapshot_ekf_mark() {
    const IMUState &st = systems_[0]->msckfvio_ptr()->imuState();
    int k = 0;
    for (int i = 0; i < 4; ++i) mark_dump.imu[k++] = st.orientation.q[i];
    for (int i = 0; i < 3; ++i) mark_dump.imu[k++] = st.position[i];
    for (int i = 0; i < 3; ++i) mark_dump.imu[k++] = st.velocity[i];
    for (int i = 0; i < 3; ++i) mark_dump.imu[k++] = st.gyro_bias[i];
    for (int i = 0; i < 3; ++i) mark_dump.imu[k++] = st.acc_bias[i];
    for (int i = 0; i < 9; ++i) mark_dump.imu[k++] = st.R_imu_cam0.m[i];
    for (int i = 0; i < 3; ++i) mark_dump.imu[k++] = st.t_cam0_imu[i];
    mark_dump.ekf_valid = true;
}

void BatchGroup::rebind_home() {
    if (!home_fe_ || !home_ekf_) return;
    ctx_ = home_fe_; ekf_ctx_ = home_ekf_;
    for (mskf_stream *s : streams_) mskf_stream_rebind(s, home_fe_, home_ekf_);
    acc_fe_ = acc_ekf_ = nullptr;
}

// front-end stage of frame k on a borrowed context (the caller has made sure nothing of this batch's front-end is in flight)
int BatchGroup::fe_stage(mskf_ctx *ctx, int k, double *acc, std::unique_ptr<FrameBatch> &out) {
    if (ctx_ != ctx) { ctx_ = ctx; for (mskf_stream *s : streams_) mskf_stream_rebind(s, ctx, nullptr); }
    acc_fe_ = acc;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = feed_imu(k, true, false);
    const auto t1 = std::chrono::steady_clock::now();
    acc[PH_IMU] += std::chrono::duration<double>(t1 - t0).count();
    if (rc == MSKF_OK) rc = step_fe(p0_.data(), p1_.data(), seq[0].on_device, t_.data(), false);
    if (rc != MSKF_OK) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    fill_handoff(k, out);
    acc[PH_HANDOFF] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t2).count();
    return MSKF_OK;
}

// filter stage of a handed-off frame on a borrowed context.  The stage ends with work it does not wait for (clone removal):
// when the next frame of this batch runs on another context, that context's queue is ordered behind it.
int BatchGroup::ekf_stage(mskf_ctx *ctx, FrameBatch *fb, double *acc) {
    if (ekf_ctx_ != ctx) { ekf_ctx_ = ctx; for (mskf_stream *s : streams_) mskf_stream_rebind(s, nullptr, ctx); }
    if (ekf_tail_ && ekf_tail_ctx_ && ekf_tail_ctx_ != ctx) { const int wrc = mskf_ctx_wait_point(ctx, ekf_tail_); if (wrc != MSKF_OK) { error_ = mskf_last_error(); return wrc; } }
    acc_ekf_ = acc;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = feed_imu(fb->frame, false, true);
    acc[PH_IMU_EKF] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc == MSKF_OK) rc = step_ekf(fb);
    if (rc != MSKF_OK) return rc;
    rc = mskf_ctx_record_point(ctx, &ekf_tail_);
    ekf_tail_ctx_ = ctx;
    if (rc != MSKF_OK) error_ = mskf_last_error();
    return rc;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void BatchGroup::set_gates(bool on) {
    mskf_ctx_timing_gate(ctx_, on ? 1 : 0);
    mskf_ctx_timing_gate(ekf_ctx_, on ? 1 : 0);
}

MultiRunner::MultiRunner(int device, int n_groups, int per_group, const mskf_calib &calib, const mskf_fe_cfg &fe, const mskf_ekf_cfg &ekf,
                         int host_threads, int ekf_host_threads)
    : n_groups_(n_groups), per_group_(per_group), off_(n_groups, 0), next_(n_groups, 0), win_(n_groups) {
    // A device offers 16 hardware queues before streams get multiplexed (GPU_MAX_HW_QUEUES): two per group, front-end and filter
    for (int g = 0; g < n_groups; ++g) groups_.emplace_back(new BatchGroup(device, per_group, calib, fe, ekf, host_threads, ekf_host_threads));
}

MultiRunner::~MultiRunner() { groups_.clear(); }

bool MultiRunner::ok() const {
    for (const auto &g : groups_) if (!g->ok()) return false;
    return !groups_.empty();
}

std::string MultiRunner::error() const {
    for (const auto &g : groups_) if (!g->error().empty()) return g->error();
    return std::string();
}

int MultiRunner::step(const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, const double *t) {
    for (int g = 0; g < n_groups_; ++g) {
        int rc = groups_[g]->step(cam0 + (size_t)g * per_group_, cam1 + (size_t)g * per_group_, on_device, t + (size_t)g * per_group_, false);
        if (rc != MSKF_OK) return rc;
    }
    return MSKF_OK;
}

int MultiRunner::run(int first, int n, bool threaded, bool pipelined) {
    if (pipelined) return run_balanced(first, 0, n, 0, nullptr, true);
    std::vector<int> rcs(n_groups_, MSKF_OK);
    auto one = [&](int g) {
        // frames [first + off, first + off + n) of the group, after catching up from where it stands
        const int from = start_of(g, first);
        next_[g] = first + off_[g] + n;
        return groups_[g]->run(from, next_[g] - from);
    };
    if (!threaded || n_groups_ == 1) {
        for (int g = 0; g < n_groups_; ++g) { rcs[g] = one(g); if (rcs[g] != MSKF_OK) return rcs[g]; }
        return MSKF_OK;
    }
    std::vector<std::thread> th;
    for (int g = 0; g < n_groups_; ++g) th.emplace_back([&, g]() { rcs[g] = one(g); });
    for (auto &t : th) t.join();
    for (int g = 0; g < n_groups_; ++g) if (rcs[g] != MSKF_OK) return rcs[g];
    return MSKF_OK;
}

int MultiRunner::run_balanced(int first, int warmup, int steps, int max_extra, double *elapsed_s, bool plain) {
    const int nb = n_groups_;
    TimedShared shared;
    shared.target_open = (long)nb * warmup;
    shared.target_close = (long)nb * (warmup + steps);
    if (plain) {     // an ordinary run: every batch does exactly its own frames (catch-up of staggered groups included), accounting on throughout
        shared.target_open = 0; shared.target_close = 0; max_extra = 0;
        for (int g = 0; g < nb; ++g) shared.target_close += first + off_[g] + warmup + steps - start_of(g, first);
        if (shared.target_close <= 0) return MSKF_OK;
    }
    if (shared.target_open <= 0) { shared.t_open = now_s(); shared.phase.store(1); }
    // per batch: frames [from, from + cnt) are its own, then it keeps going while the window is open (at most max_extra)
    struct Batch { int from = 0, cnt = 0, fe_next = 0, mark_end = 0; bool fe_busy = false, ekf_busy = false, fe_done = false; };
    std::vector<Batch> B(nb);
    for (int g = 0; g < nb; ++g) {
        B[g].from = start_of(g, first);
        B[g].cnt = first + off_[g] + warmup + steps - B[g].from;
        B[g].fe_next = B[g].from;
        B[g].mark_end = first + off_[g] + warmup + steps;
        win_[g] = TimedWindow();
        groups_[g]->set_gates(false);
        groups_[g]->mark_dump.fe_valid = groups_[g]->mark_dump.ekf_valid = false;
        groups_[g]->handoff.clear();
        for (int k = 0; k < PH_COUNT; ++k) groups_[g]->window_phase_s[k] = 0;
    }
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<int> err{MSKF_OK};
    // a worker's accounting follows the shared window at its frame boundaries; the phase times of worker w are kept in group w's
    // arrays whichever batches it ran
    static const int fe_phases[] = {PH_PUSH, PH_PREP1, PH_TRACK1, PH_AFTER1, PH_TRACK2,
                                    PH_AFTER2, PH_IMU, PH_HANDOFF, PH_FE_QWAIT};
    static const int ekf_phases[] = {PH_EKF_A, PH_UPD1, PH_EKF_B, PH_UPD2, PH_EKF_C,
                                     PH_POSVAR, PH_EKF_QWAIT, PH_IMU_EKF, PH_DIRECT};
    std::vector<mskf_ctx *> fe_ctx(nb), ekf_ctx(nb);      // worker w = the two contexts group w created (captured before any batch moves)
    for (int w = 0; w < nb; ++w) { fe_ctx[w] = groups_[w]->ctx(); ekf_ctx[w] = groups_[w]->ekf_ctx(); }
    auto gate = [&](int w, bool fe, bool on) {
        BatchGroup &G = *groups_[w];
        mskf_ctx_timing_gate(fe ? fe_ctx[w] : ekf_ctx[w], on ? 1 : 0);
        hostprof::enabled() = on;
        const int *ph = fe ? fe_phases : ekf_phases;
        const int cnt = fe ? (int)(sizeof(fe_phases) / sizeof(int)) : (int)(sizeof(ekf_phases) / sizeof(int));
        for (int k = 0; k < cnt; ++k) G.window_phase_s[ph[k]] = on ? -G.phase_s[ph[k]] : G.window_phase_s[ph[k]] + G.phase_s[ph[k]];
    };
    auto follow = [&](int w, bool fe, int &mine, double &t_begin, double &t_end) {
        const int ph = shared.phase.load(std::memory_order_acquire);
        if (mine == 0 && ph >= 1) { t_begin = now_s(); gate(w, fe, true); mine = 1; }
        if (mine == 1 && ph == 2) { t_end = now_s(); gate(w, fe, false); mine = 2; }
    };
    // Workers and batches are different things: there may be fewer workers of a kind than batches (set_workers; default one of
    // each per batch; worker w uses the contexts group w created).
    const int n_few = fe_workers_ > 0 ? std::min(nb, fe_workers_) : nb, n_ekw = ekf_workers_ > 0 ? std::min(nb, ekf_workers_) : nb;
    std::vector<std::thread> th;
    // ---- front-end workers: the batch that is furthest behind, not being worked on, with room in its hand-off queue
    for (int w = 0; w < n_few; ++w) th.emplace_back([&, w]() {
        hostprof::enabled() = false;
        int mine = 0;
        double *acc = groups_[w]->phase_s;
        TimedWindow &W = win_[w];
        for (;;) {
            int b = -1;
            {
                const double tq = now_s();
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (err.load() != MSKF_OK) return;
                    b = -1;
                    bool all_done = true;
                    for (int g = 0; g < nb; ++g) {
                        Batch &X = B[g];
                        if (X.fe_done) continue;
                        const bool own = X.fe_next < X.from + X.cnt;
                        // not while a worker is still stepping it: the filter workers leave once every batch is done, and the frame
                        // in flight would be handed off after them, never filtered (front-end one frame ahead of frames_done)
                        if (!own && !X.fe_busy && (shared.phase.load() == 2 || X.fe_next >= X.from + X.cnt + max_extra)) { X.fe_done = true; cv.notify_all(); continue; }
                        all_done = false;
                        if (X.fe_busy || groups_[g]->handoff.size() >= 2) continue;
                        if (b < 0 || X.fe_next - X.from < B[b].fe_next - B[b].from) b = g;
                    }
                    if (b >= 0 || all_done) break;
                    cv.wait(lk);
                }
                acc[PH_FE_QWAIT] += now_s() - tq;
                if (b < 0) break;
                B[b].fe_busy = true;
            }
            follow(w, true, mine, W.t_fe_begin, W.t_fe_end);
            if (mine == 1) ++W.fe_frames;
            const int k = B[b].fe_next;
            std::unique_ptr<FrameBatch> fb;
            { std::lock_guard<std::mutex> lk(mu); auto &pool = groups_[b]->handoff_pool; if (!pool.empty()) { fb = std::move(pool.back()); pool.pop_back(); } }
            const int rc = groups_[b]->fe_stage(fe_ctx[w], k, acc, fb);
            if (rc == MSKF_OK && k == B[b].mark_end - 1) groups_[b]->snapshot_fe_mark();
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc != MSKF_OK) err.store(rc);
                else { groups_[b]->handoff.push_back(std::move(fb)); ++B[b].fe_next; }
                B[b].fe_busy = false;
            }
            cv.notify_all();
            if (rc != MSKF_OK) return;
        }
        if (mine == 1) { W.t_fe_end = now_s(); gate(w, true, false); }
    });
    // ---- filter workers: the oldest handed-off frame of a batch whose filter is not being worked on
    for (int w = 0; w < n_ekw; ++w) th.emplace_back([&, w]() {
        hostprof::enabled() = false;
        int mine = 0;
        double *acc = groups_[w]->phase_s;
        TimedWindow &W = win_[w];
        for (;;) {
            int b = -1;
            std::unique_ptr<FrameBatch> fb;
            {
                const double tq = now_s();
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (err.load() != MSKF_OK) return;
                    b = -1;
                    bool pending = false;
                    for (int g = 0; g < nb; ++g) {
                        if (!B[g].fe_done || !groups_[g]->handoff.empty() || B[g].ekf_busy) pending = true;
                        if (B[g].ekf_busy || groups_[g]->handoff.empty()) continue;
                        if (b < 0 || groups_[g]->handoff.front()->frame - B[g].from < groups_[b]->handoff.front()->frame - B[b].from) b = g;
                    }
                    if (b >= 0 || !pending) break;
                    cv.wait(lk);
                }
                acc[PH_EKF_QWAIT] += now_s() - tq;
                if (b < 0) break;
                B[b].ekf_busy = true;
                fb = std::move(groups_[b]->handoff.front());
                groups_[b]->handoff.pop_front();
            }
            cv.notify_all();
            follow(w, false, mine, W.t_ekf_begin, W.t_ekf_end);
            if (mine == 1) ++W.ekf_frames;
            const int frame = fb->frame;
            const int rc = groups_[b]->ekf_stage(ekf_ctx[w], fb.get(), acc);
            if (rc == MSKF_OK && frame == B[b].mark_end - 1) groups_[b]->snapshot_ekf_mark();     // (before the batch is released to the next worker)
            {
                // the frame is through both stages: it counts.  Progress and the shared count move together under the lock, so the
                // thread that completes the closing frame sees how far every batch had got at that moment (the frames a batch
                // finishes after that are drain, done but not counted)
                std::lock_guard<std::mutex> lk(mu);
                if (rc != MSKF_OK) err.store(rc);
                else {
                    win_[b].frames_done = frame + 1 - B[b].from;
                    const long c = shared.completed.fetch_add(1) + 1;
                    if (c == shared.target_open) { shared.t_open = now_s(); shared.phase.store(1, std::memory_order_release); }
                    if (c == shared.target_close) {
                        shared.t_close = now_s(); shared.phase.store(2, std::memory_order_release);
                        for (int g = 0; g < nb; ++g) win_[g].frames_at_close = win_[g].frames_done;
                    }
                }
                groups_[b]->handoff_pool.push_back(std::move(fb));
                B[b].ekf_busy = false;
            }
            cv.notify_all();
            if (rc != MSKF_OK) return;
        }
        if (mine == 1) { W.t_ekf_end = now_s(); gate(w, false, false); }
    });
    for (auto &t : th) t.join();
    hostprof::enabled() = true;
    // every worker's queue is drained (the last clone removals are not waited for by their stage), then the batches go home
    for (int w = 0; w < nb; ++w) { mskf_ctx_sync(fe_ctx[w]); mskf_ctx_sync(ekf_ctx[w]); }
    for (int g = 0; g < nb; ++g) {
        groups_[g]->rebind_home();
        groups_[g]->set_gates(true);
        next_[g] = B[g].from + win_[g].frames_done;
    }
    if (err.load() != MSKF_OK) return err.load();
    if (shared.phase.load() != 2) return MSKF_ERR_INVALID;
    if (elapsed_s) *elapsed_s = shared.t_close - shared.t_open;
    return MSKF_OK;
}

}  // namespace cg
