// keyframes.h — a stream's stored keyframes and their matching against the stream's last frame ("Descriptor
// matching").  A keyframe is a copy of what ImageProcessor's descriptor getters return for one frame: time, feature ids,
// 32-byte descriptors, validity.  The store decides nothing: WHEN a frame becomes a keyframe and WHAT counts as a revisit is
// the caller's policy.  query() is one mskf_fe_match_batch: the query set is shared, one job per keyframe.  verify() is one
// mskf_fe_verify_batch over the hits of the last query() ("Geometric verification"): a keyframe also keeps the
// frame's published stereo observations, and the hits' id pairs become pairs of observations.  It still decides nothing.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../../include/mskf_hip.h"

namespace cg {

struct Keyframe {
    double time = 0;
    std::vector<uint64_t> ids;
    std::vector<uint8_t> desc, valid;          // 32 bytes / one byte per id
    std::vector<double> obs;                   // x0, y0, x1, y1 per id: the published undistorted normalised coordinates of that frame
};

struct KeyframeHit {
    int k = 0;                                 // index of the keyframe
    double time = 0;
    int n_matches = 0;
    std::vector<uint64_t> pairs;               // (query feature id, keyframe feature id) per accepted match, in query order
};

struct KeyframeVerification {                  // of one hit: what mskf_fe_verify returned for its pairs
    int k = 0;
    double time = 0;
    int n_matches = 0, n_usable = 0, n_inliers = 0, best = -1, status = 1;
    double R[9] = {0}, t[3] = {0}, info[36] = {0}, rms = 0;      // p_keyframe = R p_query + t in cam0 coordinates
    std::vector<uint8_t> inlier;               // one byte per pair of the hit
};

class KeyframeStore {
  public:
    int add(double time, const std::vector<uint64_t> &ids, const std::vector<uint8_t> &desc, const std::vector<uint8_t> &valid, const std::vector<double> &obs) {
        kf_.push_back(Keyframe{time, ids, desc, valid, obs});
        return (int)kf_.size() - 1;
    }
    int size() const { return (int)kf_.size(); }
    const Keyframe &at(int k) const { return kf_[k]; }
    void clear() { kf_.clear(); hits_.clear(); verified_.clear(); }
    const std::vector<KeyframeHit> &hits() const { return hits_; }          // of the last query()
    std::string refused;                       // why the store refused the last verify() ("" when it did not), for the C interface
    const std::vector<KeyframeVerification> &verified() const { return verified_; }      // of the last verify(), one per hit

    // (ids, desc, valid) against every keyframe; hits() then holds the keyframes with n_matches >= min_matches, in index order.
    // Returns the status of mskf_fe_match_batch (which refuses bad thresholds and more than 65535 descriptors in a set).
    // `time` is the time stamp of the frame the query set belongs to: verify() accepts the hits for that frame only.
    int query(mskf_ctx *ctx, double time, const std::vector<uint64_t> &ids, const std::vector<uint8_t> &desc, const std::vector<uint8_t> &valid, int max_distance, float ratio,
              bool cross_check, int min_matches) {
        hits_.clear(); verified_.clear();
        hits_time_ = time;
        if (kf_.empty()) return MSKF_OK;
        const size_t nq = ids.size();
        std::vector<mskf_fe_match_args> args(kf_.size());
        std::vector<mskf_match> m(nq * kf_.size());
        for (size_t k = 0; k < kf_.size(); ++k) {
            mskf_fe_match_args &a = args[k];
            a.nq = (int32_t)nq; a.nt = (int32_t)kf_[k].ids.size();
            a.query = desc.data(); a.query_valid = valid.data();            // the same pointers in every job: copied once
            a.train = kf_[k].desc.data(); a.train_valid = kf_[k].valid.data();
            a.max_distance = max_distance; a.ratio = ratio; a.cross_check = cross_check ? 1 : 0;
            a.matches = m.data() + nq * k; a.n_matches = 0;
        }
        const int rc = mskf_fe_match_batch(ctx, (int)args.size(), args.data());
        if (rc != MSKF_OK) return rc;
        for (size_t k = 0; k < kf_.size(); ++k) {
            if (args[k].n_matches < min_matches) continue;
            KeyframeHit h;
            h.k = (int)k; h.time = kf_[k].time; h.n_matches = args[k].n_matches;
            for (size_t i = 0; i < nq; ++i) {
                const mskf_match &r = args[k].matches[i];
                if (r.idx >= 0) { h.pairs.push_back(ids[i]); h.pairs.push_back(kf_[k].ids[(size_t)r.idx]); }
            }
            hits_.push_back(std::move(h));
        }
        return MSKF_OK;
    }

    // One mskf_fe_verify_batch with a job per hit of the last query(): the hit's id pairs as pairs of (the frame's, the keyframe's)
    // observations.  (time, ids, obs) are the frame's, as for query(); refused (MSKF_ERR_INVALID, why) when `time` is not the
    // time of the frame the hits were computed for: a newer frame has been described since, and its observations are not theirs.
    // Otherwise the status of mskf_fe_verify_batch (which refuses bad thresholds); verified() then holds one record per hit.
    int verify(mskf_ctx *ctx, double time, const std::vector<uint64_t> &ids, const std::vector<double> &obs, const double T_cam1_cam0[16], int n_hypotheses,
               uint64_t seed, double max_error, double min_depth, double max_depth, std::string &why) {
        verified_.clear();
        if (hits_.empty()) return MSKF_OK;
        if (time != hits_time_) { why = "the hits are those of another frame: query the keyframes again"; return MSKF_ERR_INVALID; }
        if (obs.size() != 4 * ids.size()) { why = "the frame has no observations"; return MSKF_ERR_INVALID; }
        std::unordered_map<uint64_t, size_t> at;
        for (size_t i = 0; i < ids.size(); ++i) at[ids[i]] = i;
        const size_t nh = hits_.size();
        std::vector<std::vector<double>> q(nh), t(nh);
        std::vector<mskf_fe_verify_args> args(nh);
        verified_.resize(nh);
        for (size_t j = 0; j < nh; ++j) {
            const KeyframeHit &h = hits_[j];
            const Keyframe &f = kf_[(size_t)h.k];
            if (f.obs.size() != 4 * f.ids.size()) { verified_.clear(); why = "a keyframe has no observations"; return MSKF_ERR_INVALID; }
            std::unordered_map<uint64_t, size_t> kat;
            for (size_t i = 0; i < f.ids.size(); ++i) kat[f.ids[i]] = i;
            const size_t m = h.pairs.size() / 2;
            q[j].resize(4 * m); t[j].resize(4 * m);
            for (size_t p = 0; p < m; ++p) {
                const auto qf = at.find(h.pairs[2 * p]);
                const auto tf = kat.find(h.pairs[2 * p + 1]);
                if (qf == at.end() || tf == kat.end()) {      // (descriptors switched off and on since the query: the frame's lists are gone)
                    verified_.clear(); why = "a matched feature is no longer among the frame's or the keyframe's: query the keyframes again"; return MSKF_ERR_INVALID;
                }
                const size_t qi = qf->second, ti = tf->second;
                for (int c = 0; c < 4; ++c) { q[j][4 * p + c] = obs[4 * qi + c]; t[j][4 * p + c] = f.obs[4 * ti + c]; }
            }
            KeyframeVerification &v = verified_[j];
            v.k = h.k; v.time = h.time; v.n_matches = h.n_matches;
            v.inlier.assign(m, 0);
            mskf_fe_verify_args &a = args[j];
            a = mskf_fe_verify_args{};
            a.n = (int32_t)m; a.n_hypotheses = n_hypotheses;
            a.query_obs = q[j].data(); a.train_obs = t[j].data(); a.usable = nullptr;
            for (int c = 0; c < 16; ++c) a.T_cam1_cam0[c] = T_cam1_cam0[c];
            a.seed = seed; a.max_error = max_error; a.min_depth = min_depth; a.max_depth = max_depth;
            a.inlier = v.inlier.data();
        }
        const int rc = mskf_fe_verify_batch(ctx, (int)nh, args.data());
        if (rc != MSKF_OK) { verified_.clear(); return rc; }
        for (size_t j = 0; j < nh; ++j) {
            KeyframeVerification &v = verified_[j];
            const mskf_fe_verify_args &a = args[j];
            v.n_usable = a.n_usable; v.n_inliers = a.n_inliers; v.best = a.best; v.status = a.status; v.rms = a.rms;
            for (int c = 0; c < 9; ++c) v.R[c] = a.R[c];
            for (int c = 0; c < 3; ++c) v.t[c] = a.t[c];
            for (int c = 0; c < 36; ++c) v.info[c] = a.info[c];
        }
        return MSKF_OK;
    }

  private:
    std::vector<Keyframe> kf_;
    std::vector<KeyframeHit> hits_;
    double hits_time_ = 0;                     // the frame the hits belong to
    std::vector<KeyframeVerification> verified_;
};

}  // namespace cg
