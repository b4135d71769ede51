// csrc/hip/fe_match.h (the header k_fe_match and the C ABI run) compiled for the host: a small shared library for
// tests/test_match_reference.py, which compares it with the numpy restatement (tests/match_reference.py).
#include <cstddef>
#include "msckf_stereo_c_amd/csrc/hip/fe_match.h"

extern "C" {
// FM_TILE, FM_MAX_N, FM_NONE, sizeof(mskf_match)
int fm_constants(int out[4]) {
    out[0] = FM_TILE; out[1] = FM_MAX_N; out[2] = (int)FM_NONE; out[3] = (int)sizeof(mskf_match);
    return 4;
}

// One job with every scan cut at `split` and merged under the header's rule (split <= 0 or >= the set's size: one part is
// empty).  Returns n_matches, or -1 for arguments the ABI would refuse.
int fm_match(const uint8_t *query, const uint8_t *query_valid, int nq, const uint8_t *train, const uint8_t *train_valid, int nt, int max_distance,
             float ratio, int cross_check, int split, mskf_match *matches) {
    if (nq < 0 || nt < 0 || nq > FM_MAX_N || nt > FM_MAX_N || (nq && (!query || !matches)) || (nt && !train)) return -1;
    if (max_distance < 0 || max_distance > FM_MAX_DISTANCE || !(ratio >= 0.f && ratio <= 1.f)) return -1;
    FeMatchDev J{};
    J.query = query; J.query_valid = query_valid; J.train = train; J.train_valid = train_valid;
    J.nq = nq; J.nt = nt; J.max_distance = max_distance; J.ratio = ratio; J.cross_check = cross_check; J.matches = matches;
    const int n = fm_match_host(J, split < 0 ? 0 : split);
    return n == fm_count_matches(matches, nq) ? n : -2;
}

// The same job at every split first .. last: the number of splits whose matches or n_matches differ from `want` / `want_n`
// (mskf_match has no padding: the records are compared as bytes).  `scratch` takes nq records.
int fm_match_splits(const uint8_t *query, const uint8_t *query_valid, int nq, const uint8_t *train, const uint8_t *train_valid, int nt, int max_distance,
                    float ratio, int cross_check, int first, int last, const mskf_match *want, int want_n, mskf_match *scratch) {
    int bad = 0;
    for (int split = first; split <= last; ++split) {
        const int n = fm_match(query, query_valid, nq, train, train_valid, nt, max_distance, ratio, cross_check, split, scratch);
        if (n != want_n || (nq && memcmp(scratch, want, sizeof(mskf_match) * (size_t)nq) != 0)) ++bad;
    }
    return bad;
}

// the merge rule on two parts given as (key, second)
void fm_merge_of(const uint32_t a[2], const uint32_t b[2], uint32_t out[2]) {
    FmPart x, y;
    x.key = a[0]; x.second = a[1]; y.key = b[0]; y.second = b[1];
    const FmPart r = fm_merge(x, y);
    out[0] = r.key; out[1] = r.second;
}

// sizeof(FeMatchDev) and the offsets of its fields, then sizeof(mskf_match) and the offsets of its fields, for the ctypes mirror
// of tests/test_gpu_match.py
int fm_match_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeMatchDev), (int)offsetof(FeMatchDev, query), (int)offsetof(FeMatchDev, query_valid), (int)offsetof(FeMatchDev, train),
                     (int)offsetof(FeMatchDev, train_valid), (int)offsetof(FeMatchDev, nq), (int)offsetof(FeMatchDev, nt), (int)offsetof(FeMatchDev, max_distance),
                     (int)offsetof(FeMatchDev, ratio), (int)offsetof(FeMatchDev, cross_check), (int)offsetof(FeMatchDev, matches),
                     (int)sizeof(mskf_match), (int)offsetof(mskf_match, idx), (int)offsetof(mskf_match, nearest), (int)offsetof(mskf_match, dist),
                     (int)offsetof(mskf_match, second)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
