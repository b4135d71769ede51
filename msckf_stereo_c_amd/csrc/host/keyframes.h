// keyframes.h — a stream's stored keyframes and their matching against the stream's last frame ("Descriptor
// matching").  A keyframe is a copy of what ImageProcessor's descriptor getters return for one frame: time, feature ids,
// 32-byte descriptors, validity.  The store decides nothing: WHEN a frame becomes a keyframe and WHAT counts as a revisit is
// the caller's policy.  query() is one mskf_fe_match_batch: the query set is shared, one job per keyframe.
#pragma once
#include <cstdint>
#include <vector>
#include "../../../include/mskf_hip.h"

namespace cg {

struct Keyframe {
    double time = 0;
    std::vector<uint64_t> ids;
    std::vector<uint8_t> desc, valid;          // 32 bytes / one byte per id
};

struct KeyframeHit {
    int k = 0;                                 // index of the keyframe
    double time = 0;
    int n_matches = 0;
    std::vector<uint64_t> pairs;               // (query feature id, keyframe feature id) per accepted match, in query order
};

class KeyframeStore {
  public:
    int add(double time, const std::vector<uint64_t> &ids, const std::vector<uint8_t> &desc, const std::vector<uint8_t> &valid) {
        kf_.push_back(Keyframe{time, ids, desc, valid});
        return (int)kf_.size() - 1;
    }
    int size() const { return (int)kf_.size(); }
    const Keyframe &at(int k) const { return kf_[k]; }
    void clear() { kf_.clear(); hits_.clear(); }
    const std::vector<KeyframeHit> &hits() const { return hits_; }          // of the last query()

    // (ids, desc, valid) against every keyframe; hits() then holds the keyframes with n_matches >= min_matches, in index order.
    // Returns the status of mskf_fe_match_batch (which refuses bad thresholds and more than 65535 descriptors in a set).
    int query(mskf_ctx *ctx, const std::vector<uint64_t> &ids, const std::vector<uint8_t> &desc, const std::vector<uint8_t> &valid, int max_distance, float ratio,
              bool cross_check, int min_matches) {
        hits_.clear();
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

  private:
    std::vector<Keyframe> kf_;
    std::vector<KeyframeHit> hits_;
};

}  // namespace cg
