// fe_match.h — the opt-in brute-force Hamming matcher of the 256-bit descriptors of fe_brief.h ("Descriptor
// matching").  ONE source: the kernel of fe_match.hip, the C ABI (mskf_fe_match*) and the g++-compiled CPU harness
// (tests/cpp/fe_match_test.cpp) all run these functions.  Everything is integer arithmetic but the ratio test, which is one
// float32 multiplication and one comparison.
//   job       nq query and nt train descriptors of FM_BYTES bytes, 0 <= nq, nt <= FM_MAX_N; per set an optional validity array,
//             one byte per descriptor, != 0 = valid, null = all valid;
//   distance  d(i, j) = popcount of the XOR of the FM_BYTES bytes, 0 .. 256;
//   key       (d << 16) | index: 32 bits whose minimum is the smallest (distance, index) pair; FM_KEY_NONE = nothing seen;
//   forward   for a valid query i: nearest = the valid train j of the smallest key, dist = d(i, nearest), second = the
//             smallest d(i, j) over valid j != nearest (it may equal dist);
//   none      no valid train, or an invalid query: nearest = -1, dist = second = FM_NONE; one valid train: second = FM_NONE;
//   backward  bwd(j) = the valid query i of the smallest key (d(i, j) << 16) | i; asked only with cross_check != 0;
//   accept    idx = nearest iff nearest >= 0, dist <= max_distance (0 .. 256), the ratio test holds (ratio == 0: off;
//             second == FM_NONE: passes; else (float)dist < ratio * (float)second in float32, ratio in (0, 1]) and, with
//             cross_check != 0, bwd(nearest) == i; otherwise idx = -1.  The thresholds apply to the forward direction only;
//   count     n_matches = the number of queries with idx >= 0;
//   merge     two partial results over disjoint ranges of the scanned set: best = the smaller key, second = the smallest of
//             the losing key's distance and the two seconds (fm_merge).  A scan is that merge over one-element parts, so the
//             result does not depend on how the range is cut or in which order the parts meet.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../../include/mskf_types.h"

#if defined(__HIPCC__)
#define FMT_FN __host__ __device__ __forceinline__
#else
#define FMT_FN inline
#endif

#define FM_BYTES 32
#define FM_WORDS 8                                   // 32-bit words of a descriptor
#define FM_MAX_N 65535                               // an index fits 16 bits
#define FM_NONE 0xFFFFu                              // dist / second without a neighbour
#define FM_KEY_NONE 0xFFFFFFFFu
#define FM_TILE 256                                  // descriptors of the scanned set the kernel stages at a time
#define FM_MAX_DISTANCE (8 * FM_BYTES)               // 256

static_assert(sizeof(mskf_match) == 12, "mskf_match is 12 bytes");

// One job of a k_fe_match launch.  query and train are 16-byte aligned (the kernel loads them 16 bytes at a time); the
// validity arrays and matches need no alignment.  nq == 0: skipped.
struct FeMatchDev {
    const uint8_t *query, *query_valid;   // 32 nq bytes; nq bytes or null
    const uint8_t *train, *train_valid;   // 32 nt bytes; nt bytes or null
    int nq, nt;
    int max_distance;                     // 0 .. 256
    float ratio;                          // 0 = off, else (0, 1]
    int cross_check, pad_;
    mskf_match *matches;                  // out: nq records
};

// ---- distance
FMT_FN uint32_t fm_distance(const uint32_t a[FM_WORDS], const uint32_t b[FM_WORDS]) {
    uint32_t d = 0;
    for (int k = 0; k < FM_WORDS; ++k) d += (uint32_t)__builtin_popcount(a[k] ^ b[k]);
    return d;
}

// ---- a partial result over part of the scanned set
struct FmPart { uint32_t key, second; };              // FM_KEY_NONE / FM_NONE: nothing / no other seen

FMT_FN FmPart fm_part_none() { FmPart p; p.key = FM_KEY_NONE; p.second = FM_NONE; return p; }
FMT_FN uint32_t fm_key(uint32_t d, uint32_t index) { return (d << 16) | index; }
FMT_FN uint32_t fm_key_dist(uint32_t key) { return key >> 16; }          // (FM_KEY_NONE gives FM_NONE)

FMT_FN FmPart fm_merge(FmPart a, FmPart b) {
    const uint32_t lose = fm_key_dist(a.key < b.key ? b.key : a.key);
    uint32_t s = a.second < b.second ? a.second : b.second;
    FmPart r;
    r.key = a.key < b.key ? a.key : b.key;
    r.second = lose < s ? lose : s;
    return r;
}
// the element (d, index) joins: a merge with the part that holds it alone
FMT_FN FmPart fm_insert(FmPart p, uint32_t d, uint32_t index) {
    FmPart e; e.key = fm_key(d, index); e.second = FM_NONE;
    return fm_merge(p, e);
}

// ---- acceptance of a forward result (the cross-check comes on top)
FMT_FN bool fm_accept(FmPart p, int max_distance, float ratio) {
    if (p.key == FM_KEY_NONE) return false;
    const uint32_t d = fm_key_dist(p.key);
    if (d > (uint32_t)max_distance) return false;
    if (ratio == 0.f || p.second == FM_NONE) return true;
    return (float)d < ratio * (float)p.second;
}

FMT_FN mskf_match fm_result(FmPart p, bool accepted) {
    mskf_match m;
    m.nearest = p.key == FM_KEY_NONE ? -1 : (int32_t)(p.key & 0xFFFFu);
    m.idx = accepted ? m.nearest : -1;
    m.dist = (uint16_t)fm_key_dist(p.key);
    m.second = (uint16_t)p.second;
    return m;
}

// ---- a job on the host (the harness; the kernel does the same with one query per lane and the scanned set cut over its
// wavefronts).  `own` against set[j0 .. j1): the part.
inline FmPart fm_scan_host(const uint8_t *own, const uint8_t *set, const uint8_t *valid, int j0, int j1) {
    uint32_t a[FM_WORDS], b[FM_WORDS];
    memcpy(a, own, FM_BYTES);
    FmPart p = fm_part_none();
    for (int j = j0; j < j1; ++j) {
        if (valid && !valid[j]) continue;
        memcpy(b, set + (size_t)FM_BYTES * j, FM_BYTES);
        p = fm_insert(p, fm_distance(a, b), (uint32_t)j);
    }
    return p;
}
// `own` against the whole set, as the merge of the parts before and from `split` (0 <= split <= n)
inline FmPart fm_scan_split_host(const uint8_t *own, const uint8_t *set, const uint8_t *valid, int n, int split) {
    return fm_merge(fm_scan_host(own, set, valid, 0, split), fm_scan_host(own, set, valid, split, n));
}
// The job J with host pointers; every scan is cut at `split` (clamped to the scanned set's size).  Returns n_matches.
inline int fm_match_host(const FeMatchDev &J, int split) {
    int n_matches = 0;
    std::vector<int32_t> bwd(J.cross_check ? (size_t)J.nt : 0, -1);          // bwd(j), scanned when first asked for (the kernel scans per query)
    for (int i = 0; i < J.nq; ++i) {
        FmPart p = fm_part_none();
        if (!J.query_valid || J.query_valid[i])
            p = fm_scan_split_host(J.query + (size_t)FM_BYTES * i, J.train, J.train_valid, J.nt, split < J.nt ? split : J.nt);
        bool ok = fm_accept(p, J.max_distance, J.ratio);
        if (ok && J.cross_check) {
            const uint32_t j = p.key & 0xFFFFu;
            if (bwd[j] < 0)                               // (the query i itself is valid and in the scan: the part holds a key)
                bwd[j] = (int32_t)(fm_scan_split_host(J.train + (size_t)FM_BYTES * j, J.query, J.query_valid, J.nq, split < J.nq ? split : J.nq).key & 0xFFFFu);
            ok = bwd[j] == i;
        }
        J.matches[i] = fm_result(p, ok);
        n_matches += ok ? 1 : 0;
    }
    return n_matches;
}
inline int fm_count_matches(const mskf_match *m, int nq) {
    int n = 0;
    for (int i = 0; i < nq; ++i) n += m[i].idx >= 0 ? 1 : 0;
    return n;
}
