// mskf_capi_fe.cpp — C-ABI: the per-frame front end: stream settings, push, cell maxima, track and the device frame (include/mskf_hip.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <chrono>
#include <initializer_list>
#include <vector>
#include "mskf_internal.h"

void fill_pyr(const mskf_stream *s, int idx, PyrDev &p) {
    for (int l = 0; l < MSKF_LEVELS; ++l) {
        p.lvl[l] = s->pyr[idx] + s->lvl_off[l];
        p.w[l] = s->lw[l];
        p.h[l] = s->lh[l];
    }
    p.lvl[0] = level0(s, idx);
}

static void fill_fe_desc(const mskf_stream *s, FeStreamDev &d) {
    std::memset(&d, 0, sizeof(d));
    fill_pyr(s, s->i_prev0, d.prev0);
    fill_pyr(s, s->i_curr0, d.curr0);
    fill_pyr(s, s->i_curr1, d.curr1);
    d.cam0 = s->cam0; d.cam1 = s->cam1;
    std::memcpy(d.R01, s->R01, sizeof(d.R01));
    std::memcpy(d.E, s->E, sizeof(d.E));
    d.epi_thresh = s->epi_thresh;
    d.det_rows = s->fe.det_rows; d.det_cols = s->fe.det_cols; d.cell_w = s->det_cw; d.cell_h = s->det_ch;
    d.det_floor = s->det_floor;
    d.cell_keys = (unsigned long long *)(s->ctx->cell_arena.d + s->cell_off);
}

// The descriptor of the stream's current pair as every launch of this file stages it: pyramids, camera models, R01, E, epi_thresh
// and the detector's cells; Hpred and the point fields are zero (the caller's).  No HIP call, no state changed.
extern "C" int fe_stream_desc(const mskf_stream *s, FeStreamDev *out) {
    if (!s || !out || !s->has_curr) return MSKF_ERR_INVALID;
    fill_fe_desc(s, *out);
    return MSKF_OK;
}

// The push generation as the 8-bit tag the cell keys carry in their top byte (1 .. 255; 0 is "never written").
static inline unsigned int push_gen_tag(unsigned long long push_gen) { return (unsigned int)((push_gen - 1) % 255ULL) + 1U; }
static inline size_t cell_key_bytes(const mskf_stream *s) { return sizeof(unsigned long long) * (size_t)s->fe.det_rows * s->fe.det_cols; }

// The last step of a setter that replaces device blocks of a stream (the opt-in settings below: cold paths, called outside a run).
// Launches that still read old blocks finish first -- the whole device, since the stream may have been pushed on another context
// before a rebind (mskf_stream_rebind) -- then the old blocks are freed; if that wait fails, the fresh ones are, and the stream stays.
static int replace_blocks(std::initializer_list<void *> old, std::initializer_list<void *> fresh) {
    bool any = false;
    for (void *p : old) any = any || p;
    if (!any) return MSKF_OK;
    const hipError_t e = hipDeviceSynchronize();
    for (void *p : e == hipSuccess ? old : fresh) if (p) (void)hipFree(p);
    if (e == hipSuccess) return MSKF_OK;
    mskf_set_error(hipGetErrorString(e));
    return MSKF_ERR_HIP;
}

// ---- opt-in equalisation of pushed images (include/mskf_hip.h; arithmetic and job layout: fe_equalize.h)
static int eq_validate(const mskf_stream *s, const mskf_fe_equalize *cfg) {
    if (!s || !cfg) return MSKF_ERR_INVALID;
    if (cfg->mode != EQ_OFF && cfg->mode != EQ_GLOBAL && cfg->mode != EQ_CLAHE) { mskf_set_error("equalize: unknown mode (0 off, 1 global, 2 CLAHE)"); return MSKF_ERR_INVALID; }
    if (cfg->tiles_x < 1 || cfg->tiles_y < 1) { mskf_set_error("equalize: tiles_x and tiles_y must be at least 1"); return MSKF_ERR_INVALID; }
    if (cfg->tiles_x > s->w || cfg->tiles_y > s->h) { mskf_set_error("equalize: more tiles than pixels in a dimension"); return MSKF_ERR_INVALID; }
    if (!std::isfinite(cfg->clip_limit) || cfg->clip_limit < 0.0) { mskf_set_error("equalize: clip_limit must be finite and not negative"); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_equalize(mskf_stream *s, const mskf_fe_equalize *cfg) {
    if (const int rc = eq_validate(s, cfg)) return rc;        // no HIP call before this
    mskf_stream::Equalize E;                                   // everything is decided here, the stream changes at the end
    E.cfg = *cfg; E.cfg._pad = 0;
    size_t lut_bytes = 0, part_bytes = 0;
    if (cfg->mode == EQ_CLAHE) {
        E.geom = eq_geometry(s->w, s->h, cfg->tiles_x, cfg->tiles_y);
        E.clip = eq_clip(cfg->clip_limit, E.geom.tw * E.geom.th);
        lut_bytes = 256 * (size_t)cfg->tiles_x * cfg->tiles_y;
    } else if (cfg->mode == EQ_GLOBAL) {
        E.strip_rows = eq_strip_rows(s->h);
        E.n_strips = (s->h + E.strip_rows - 1) / E.strip_rows;
        lut_bytes = 256;
        part_bytes = sizeof(int) * 256 * (size_t)E.n_strips;
    }
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    if (lut_bytes) {
        MSKF_HIPCHK(hipMalloc((void **)&E.mem, 2 * (lut_bytes + part_bytes)));
        for (int c = 0; c < 2; ++c) {
            E.lut[c] = (uint8_t *)E.mem + c * lut_bytes;
            E.part[c] = part_bytes ? (int *)(E.mem + 2 * lut_bytes + c * part_bytes) : nullptr;
        }
    }
    if (const int rc = replace_blocks({s->eq.mem}, {E.mem})) return rc;
    s->eq = E;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_equalize(mskf_stream *s, mskf_fe_equalize *out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    *out = s->eq.cfg;
    return MSKF_OK;
}

// The equalising images of a push: their jobs, and the grid that covers the largest of them.
struct EqLaunch {
    int n = 0, max_units = 1, any_global = 0, max_regions = 1, splits = 1;
    void add(EqJob *jobs, const mskf_stream *s, int cam, const uint8_t *src, uint8_t *dst) {
        const mskf_stream::Equalize &E = s->eq;
        EqJob &j = jobs[n++];
        j.src = src; j.dst = dst; j.part = E.part[cam]; j.lut = E.lut[cam];
        j.w = s->w; j.h = s->h; j.mode = E.cfg.mode;
        j.tiles_x = E.cfg.tiles_x; j.tiles_y = E.cfg.tiles_y; j.tw = E.geom.tw; j.th = E.geom.th; j.clip = E.clip;
        j.strip_rows = E.strip_rows; j.n_strips = E.n_strips; j._pad = 0;
        const bool clahe = j.mode == EQ_CLAHE;
        max_units = std::max(max_units, clahe ? j.tiles_x * j.tiles_y : j.n_strips);
        any_global |= clahe ? 0 : 1;
        max_regions = std::max(max_regions, eq_regions(j.mode, j.tiles_x, j.tiles_y));
        // a workgroup of the apply kernel takes about 4096 pixels (sixteen per lane) of its region: a region is about a tile
        const int rw = clahe ? j.tw : j.w, rh = clahe ? j.th : j.h, rows = std::max(1, 4096 / std::max(rw, 1));
        splits = std::max(splits, std::min(64, (rh + rows - 1) / rows));
    }
};

// ---- opt-in input pixel formats (include/mskf_hip.h; arithmetic and job layout: fe_pixfmt.h)
static inline size_t px_raw_bytes(const mskf_stream *s) { return (size_t)s->w * s->h * s->px.bpp; }      // one camera's raw raster, dense

static int px_validate(const mskf_stream *s, const mskf_fe_input_format *cfg) {
    if (!s || !cfg) return MSKF_ERR_INVALID;
    if (px_bpp(cfg->format) == 0) { mskf_set_error("input format: unknown format (MSKF_PIX_GRAY8 .. MSKF_PIX_BAYER_BGGR8)"); return MSKF_ERR_INVALID; }
    if (cfg->shift < 0 || cfg->shift > PX_MAX_SHIFT) { mskf_set_error("input format: shift must be 0 .. 8"); return MSKF_ERR_INVALID; }
    if (cfg->shift != 0 && cfg->format != PX_GRAY16) { mskf_set_error("input format: a shift other than 0 goes with MSKF_PIX_GRAY16 only"); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_input_format(mskf_stream *s, const mskf_fe_input_format *cfg) {
    if (const int rc = px_validate(s, cfg)) return rc;        // no HIP call before this
    mskf_stream::PixFmt X;                                     // everything is decided here, the stream changes at the end
    X.cfg = *cfg; X.bpp = px_bpp(cfg->format);
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    if (cfg->format != PX_GRAY8) MSKF_HIPCHK(hipMalloc((void **)&X.raw, 2 * (size_t)s->w * s->h * X.bpp));
    if (const int rc = replace_blocks({s->px.raw}, {X.raw})) return rc;
    s->px = X;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_input_format(mskf_stream *s, mskf_fe_input_format *out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    *out = s->px.cfg;
    return MSKF_OK;
}

// ---- opt-in image masks (include/mskf_hip.h; erosion, packing and the gate: fe_mask.h)
static int mask_validate(const mskf_stream *s, const mskf_fe_mask *cfg) {
    if (!s) return MSKF_ERR_INVALID;
    if (!cfg) { mskf_set_error("mask: null configuration"); return MSKF_ERR_INVALID; }
    if (cfg->cam0 || cfg->cam1) {
        if (cfg->width != s->w || cfg->height != s->h) { mskf_set_error("mask: size differs from the stream's level 0"); return MSKF_ERR_INVALID; }
        if (cfg->pitch < cfg->width) { mskf_set_error("mask: pitch below the width"); return MSKF_ERR_INVALID; }
        if (cfg->margin < 0 || cfg->margin > FM_MAX_MARGIN) { mskf_set_error("mask: margin must be 0 .. 64"); return MSKF_ERR_INVALID; }
    }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_mask(mskf_stream *s, const mskf_fe_mask *cfg) {
    if (const int rc = mask_validate(s, cfg)) return rc;      // no HIP call before this
    mskf_stream::Mask M;                                       // everything is decided here, the stream changes at the end
    const uint8_t *const src[2] = {cfg->cam0, cfg->cam1};
    const size_t words = (size_t)s->h * fm_pitch_words(s->w);
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    if (src[0] || src[1]) {
        M.margin = cfg->margin;
        std::vector<uint8_t> usable((size_t)s->w * s->h);
        for (int c = 0; c < 2; ++c) {
            if (!src[c]) continue;
            fm_erode(src[c], (size_t)cfg->pitch, s->w, s->h, cfg->margin, usable.data());
            M.host[c].resize(words);
            fm_pack(usable.data(), s->w, s->h, M.host[c].data());
            hipError_t e = hipMalloc((void **)&M.dev[c], sizeof(uint32_t) * words);
            if (e == hipSuccess) e = hipMemcpy(M.dev[c], M.host[c].data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice);     // (caller memory's image: as set_cov)
            if (e != hipSuccess) {
                for (int k = 0; k < 2; ++k) if (M.dev[k]) (void)hipFree(M.dev[k]);
                mskf_set_error(hipGetErrorString(e));
                return MSKF_ERR_HIP;
            }
        }
    }
    if (const int rc = replace_blocks({s->mask.dev[0], s->mask.dev[1]}, {M.dev[0], M.dev[1]})) return rc;
    s->mask = std::move(M);
    return MSKF_OK;
}

extern "C" int mskf_fe_get_mask(mskf_stream *s, int cam, uint8_t *out, int capacity, int *w, int *h, int *margin) {
    if (!s || cam < 0 || cam > 1 || !w || !h) return MSKF_ERR_INVALID;
    if (margin) *margin = s->mask.margin;
    if (!s->mask.dev[cam]) { *w = 0; *h = 0; return MSKF_OK; }
    if (!out) return MSKF_ERR_INVALID;
    if ((long long)capacity < (long long)s->w * s->h) return MSKF_ERR_CAPACITY;
    fm_unpack(s->mask.host[cam].data(), s->w, s->h, out);
    *w = s->w; *h = s->h;
    return MSKF_OK;
}

// One opt-in setting of the streams of a launch, element for element beside its descriptors.  *any comes in as what the caller
// already knows (false, or true: stage it whatever the streams say) and goes out true when a stream wants(); while it is false
// nothing is touched, else A is grown to n, fill() writes every stream's element and *cp is the array's staging copy.
template <typename T, typename Wants, typename Fill>
static int stage_beside(PinnedDev<T> &A, int n, mskf_stream *const *streams, Wants wants, Fill fill, MskfCopy *cp, bool *any) {
    for (int i = 0; i < n && !*any; ++i) *any = wants(*streams[i]);
    if (!*any) return MSKF_OK;
    if (const int rc = A.ensure(n)) return rc;
    for (int i = 0; i < n; ++i) fill(*streams[i], A.h[i]);
    *cp = MskfCopy{A.d, A.h, sizeof(T) * (size_t)n};
    return MSKF_OK;
}

// The masks a launch looks at (cam0_only: the detector of a push, which = 0; else a track pass, which = 1), in mask_desc[which].
static int stage_masks(mskf_ctx *ctx, int which, int n, mskf_stream *const *streams, bool cam0_only, MskfCopy *cp, bool *any) {
    return stage_beside(ctx->mask_desc[which], n, streams,
                        [&](const mskf_stream &s) { return s.mask.dev[0] || (!cam0_only && s.mask.dev[1]); },
                        [&](const mskf_stream &s, FeMaskDev &d) { d = FeMaskDev{s.mask.dev[0], cam0_only ? nullptr : s.mask.dev[1], fm_pitch_words(s.w), 0}; }, cp, any);
}

// ---- opt-in ZNCC patch check of tracks and stereo matches (include/mskf_hip.h; arithmetic and the gate: fe_patch.h)
static int patch_validate(const mskf_stream *s, const mskf_fe_patch_check *cfg) {
    if (!s) return MSKF_ERR_INVALID;
    if (!cfg) { mskf_set_error("patch check: null configuration"); return MSKF_ERR_INVALID; }
    if (cfg->mode & ~(FP_TEMPORAL | FP_STEREO)) { mskf_set_error("patch check: unknown mode bit (1 temporal, 2 stereo)"); return MSKF_ERR_INVALID; }
    if (cfg->mode != 0 && (cfg->half < FP_MIN_HALF || cfg->half > FP_MAX_HALF)) { mskf_set_error("patch check: half must be 2 .. 7"); return MSKF_ERR_INVALID; }
    for (const float t : {cfg->min_zncc_temporal, cfg->min_zncc_stereo})
        if (!std::isfinite(t) || t < 0.f || t > 1.f) { mskf_set_error("patch check: a threshold must lie in [0, 1]"); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_patch_check(mskf_stream *s, const mskf_fe_patch_check *cfg) {
    if (const int rc = patch_validate(s, cfg)) return rc;
    s->patch = *cfg;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_patch_check(mskf_stream *s, mskf_fe_patch_check *out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    *out = s->patch;
    return MSKF_OK;
}

// A stream's element of patch_desc (the track pass stages it).
static void patch_fill(const mskf_stream &s, FePatchDev &d) {
    const mskf_fe_patch_check &c = s.patch;
    d = FePatchDev{fp_thr2(c.min_zncc_temporal), fp_thr2(c.min_zncc_stereo), c.half, c.mode};
}

// ---- opt-in forward-backward check of tracks and stereo matches (include/mskf_hip.h; the decision: fe_fb.h, the kernel: fe_fb.hip)
static int fb_validate(const mskf_stream *s, const mskf_fe_fb_check *cfg) {
    if (!s) return MSKF_ERR_INVALID;
    if (!cfg) { mskf_set_error("forward-backward check: null configuration"); return MSKF_ERR_INVALID; }
    if (cfg->mode & ~(FB_TEMPORAL | FB_STEREO)) { mskf_set_error("forward-backward check: unknown mode bit (1 temporal, 2 stereo)"); return MSKF_ERR_INVALID; }
    for (const float t : {cfg->max_error_temporal, cfg->max_error_stereo})
        if (!std::isfinite(t) || t < 0.f || t > FB_MAX_ERROR) { mskf_set_error("forward-backward check: a threshold must lie in [0, 64] pixels"); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_fb_check(mskf_stream *s, const mskf_fe_fb_check *cfg) {
    if (const int rc = fb_validate(s, cfg)) return rc;
    s->fb = *cfg;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_fb_check(mskf_stream *s, mskf_fe_fb_check *out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    *out = s->fb;
    return MSKF_OK;
}

// A stream's element of fb_desc (the track pass stages it).
static void fb_fill(const mskf_stream &s, FeFbDev &d) {
    const mskf_fe_fb_check &c = s.fb;
    d = FeFbDev{fb_thr2(c.max_error_temporal), fb_thr2(c.max_error_stereo), c.mode};
}

// ---- opt-in camera models (include/mskf_hip.h; arithmetic, domains and the coefficient check: fe_cam_models.h)
static int cam_validate(const mskf_stream *s, const mskf_fe_camera_model *cfg) {
    if (!s) return MSKF_ERR_INVALID;
    if (!cfg) { mskf_set_error("camera model: null configuration"); return MSKF_ERR_INVALID; }
    if (cfg->cam != 0 && cfg->cam != 1) { mskf_set_error("camera model: cam must be 0 or 1"); return MSKF_ERR_INVALID; }
    static const char *const why[] = {nullptr, "camera model: unknown model (0 radtan, 1 equidistant, 2 radtan8, 3 fov, 4 ds)", "camera model: a coefficient is not finite",
                                      "camera model: fov's w must lie in (0, pi)", "camera model: ds's xi must lie in (-1, 1]", "camera model: ds's alpha must lie in [0, 1]"};
    if (const int bad = fcm_validate(cfg->model, cfg->coeffs)) { mskf_set_error(why[bad]); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_camera_model(mskf_stream *s, const mskf_fe_camera_model *cfg) {
    if (const int rc = cam_validate(s, cfg)) return rc;
    const int c = cfg->cam;
    s->cam_ext.model[c] = cfg->model;
    std::memcpy(s->cam_ext.coef[c], cfg->coeffs, sizeof(cfg->coeffs));
    if (cfg->model < FCM_RADTAN8) {      // back on the base path: CamDev is what k_track4 reads
        CamDev &cam = c ? s->cam1 : s->cam0;
        cam.model = cfg->model;
        std::memcpy(cam.D, cfg->coeffs, sizeof(cam.D));
    }
    return MSKF_OK;
}

extern "C" int mskf_fe_get_camera_model(mskf_stream *s, int cam, mskf_fe_camera_model *out) {
    if (!s || !out || (cam != 0 && cam != 1)) return MSKF_ERR_INVALID;
    out->cam = cam; out->model = s->cam_ext.model[cam];
    std::memcpy(out->coeffs, s->cam_ext.coef[cam], sizeof(out->coeffs));
    return MSKF_OK;
}

// A stream's element of cam_desc (the track pass stages it).
static void cam_fill(const mskf_stream &s, FeCamExtDev &d) {
    d.model[0] = s.cam_ext.model[0]; d.model[1] = s.cam_ext.model[1];
    std::memcpy(d.coef, s.cam_ext.coef, sizeof(s.cam_ext.coef));
}

// ---- opt-in deeper LK pyramids (include/mskf_hip.h; the size chain and the validity rule: fe_deep.h, the pyramid kernel: fe_deep.hip)
static int deep_validate(const mskf_stream *s, int levels) {
    if (!s) return MSKF_ERR_INVALID;
    const int bad = fd_validate(s->w, s->h, levels);
    if (bad == 1) { mskf_set_error("lk levels: must be 4 .. 8"); return MSKF_ERR_INVALID; }
    if (bad == 2) {
        mskf_set_error("lk levels: " + std::to_string(levels) + " levels need a top level of at least 15 x 15 pixels; a " + std::to_string(s->w) + " x " +
                       std::to_string(s->h) + " image allows at most " + std::to_string(fd_max_levels(s->w, s->h)));
        return MSKF_ERR_INVALID;
    }
    if (s->push_gen != 0) { mskf_set_error("lk levels: can be set only before the stream's first push"); return MSKF_ERR_INVALID; }
    return mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE);
}

extern "C" int mskf_fe_set_lk_levels(mskf_stream *s, int levels) {
    if (const int rc = deep_validate(s, levels)) return rc;    // no HIP call before this
    mskf_stream::Deep D;                                       // everything is decided here, the stream changes at the end
    D.levels = levels;
    int w = s->lw[MSKF_LEVELS - 1], h = s->lh[MSKF_LEVELS - 1];
    for (int l = MSKF_LEVELS; l < levels; ++l) {
        w = fd_half(w); h = fd_half(h);
        const int k = l - MSKF_LEVELS;
        D.w[k] = w; D.h[k] = h; D.off[k] = D.plane_bytes;
        D.plane_bytes += round_up((size_t)w * h, 64);
    }
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    if (D.plane_bytes) MSKF_HIPCHK(hipMalloc((void **)&D.mem, 3 * D.plane_bytes));
    if (const int rc = replace_blocks({s->deep.mem}, {D.mem})) return rc;
    s->deep = D;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_lk_levels(mskf_stream *s, int *levels) {
    if (!s || !levels) return MSKF_ERR_INVALID;
    *levels = s->deep.levels;
    return MSKF_OK;
}

static void fill_deep_pyr(const mskf_stream *s, int idx, PyrDeepDev &p) {
    for (int l = MSKF_LEVELS; l < s->deep.levels; ++l) {
        const int k = l - MSKF_LEVELS;
        p.lvl[k] = s->deep.level(idx, l); p.w[k] = s->deep.w[k]; p.h[k] = s->deep.h[k];
    }
}

// A stream's element of deep_desc (the track pass stages it).
static void deep_fill(const mskf_stream &s, FeDeepDev &d) {
    std::memset(&d, 0, sizeof(d));
    d.levels = s.deep.levels;
    fill_deep_pyr(&s, s.i_prev0, d.prev0); fill_deep_pyr(&s, s.i_curr0, d.curr0); fill_deep_pyr(&s, s.i_curr1, d.curr1);
}

// ---- the track pass: a track launch over the descriptors of a batch with everything the streams' opt-in settings add to it.
// plan_track_pass stages the settings a stream of the batch has, run_track_pass enqueues the kernels; a track batch runs one
// pass, a device frame two (both over the same staged arrays).  A new per-stream option of the track is a fill function beside
// its setter, a flag here, a line in the plan and a line in the run.
struct TrackPass {
    bool masked = false;             // a stream has an image mask: the mask gate runs
    bool patch_checked = false;      // ... a patch check: the patch gate runs
    bool fb_checked = false;         // ... a forward-backward check: its gate runs
    bool deep = false;               // ... more than four LK levels: the deep instantiations of the track kernel and of that gate run
    bool cams_staged = false;        // ... an extended camera model, or the pass is deep: the extended instantiation runs (unless deep)
    static constexpr int kMaxSegs = 5;
    MskfCopy seg[kMaxSegs];          // the staging copies of what was staged: the caller appends them to its own segments
    int n_seg = 0;
};

// No HIP call but the arenas' growth.  With no option on any stream of the batch nothing is touched and no segment is added.
static int plan_track_pass(mskf_ctx *ctx, int n, mskf_stream *const *streams, TrackPass &P) {
    int rc;
    if ((rc = stage_masks(ctx, 1, n, streams, false, &P.seg[P.n_seg], &P.masked)) != MSKF_OK) return rc;
    P.n_seg += P.masked;
    if ((rc = stage_beside(ctx->patch_desc, n, streams, [](const mskf_stream &s) { return s.patch.mode != 0; }, patch_fill, &P.seg[P.n_seg], &P.patch_checked)) != MSKF_OK) return rc;
    P.n_seg += P.patch_checked;
    if ((rc = stage_beside(ctx->fb_desc, n, streams, [](const mskf_stream &s) { return s.fb.mode != 0; }, fb_fill, &P.seg[P.n_seg], &P.fb_checked)) != MSKF_OK) return rc;
    P.n_seg += P.fb_checked;
    if ((rc = stage_beside(ctx->deep_desc, n, streams, [](const mskf_stream &s) { return s.deep.any(); }, deep_fill, &P.seg[P.n_seg], &P.deep)) != MSKF_OK) return rc;
    P.n_seg += P.deep;
    // the deep instantiation of the track kernel reads the camera models too: a deep pass stages them whatever they are
    P.cams_staged = P.deep;
    if ((rc = stage_beside(ctx->cam_desc, n, streams, [](const mskf_stream &s) { return s.cam_ext.any(); }, cam_fill, &P.seg[P.n_seg], &P.cams_staged)) != MSKF_OK) return rc;
    P.n_seg += P.cams_staged;
    return MSKF_OK;
}

// The pass over `desc_dev`: temporal track -> bounds gate + stereo guess -> stereo track -> gates + undistortion in one launch
// (k_track4; its extended instantiation over cam_desc; its deep one over cam_desc and deep_desc), timed as MSKF_K_LK with units 0
// (the _end sets them); then the point gates in the order mask, patch, forward-backward, each over the survivors of those before
// it and timed under its own kind.  Returns the track launch's timing slot.
static int run_track_pass(mskf_ctx *ctx, const TrackPass &P, const FeStreamDev *desc_dev, int n, int max_pts) {
    hipStream_t st = ctx->stream;
    const int ts = mskf_t_begin(ctx, MSKF_K_LK);
    if (P.deep) fe_launch_track_deep(desc_dev, ctx->cam_desc.d, ctx->deep_desc.d, n, max_pts, st);
    else if (P.cams_staged) fe_launch_track_ext(desc_dev, ctx->cam_desc.d, n, max_pts, st);
    else fe_launch_track(desc_dev, n, max_pts, st);
    mskf_t_end(ctx, ts, 0);
    const auto gate = [&](bool on, int kind, auto launch) {
        if (!on) return;
        const int t = mskf_t_begin(ctx, kind);
        launch();
        mskf_t_end(ctx, t, n);
    };
    gate(P.masked, MSKF_K_FE_MASK, [&] { fe_launch_mask_points(desc_dev, ctx->mask_desc[1].d, n, max_pts, st); });
    gate(P.patch_checked, MSKF_K_FE_PATCH, [&] { fe_launch_patch_points(desc_dev, ctx->patch_desc.d, n, max_pts, st); });
    gate(P.fb_checked, MSKF_K_FE_FB, [&] {
        if (P.deep) fe_launch_fb_points_deep(desc_dev, ctx->fb_desc.d, ctx->deep_desc.d, n, max_pts, st);      // (a backward track has its forward track's depth)
        else fe_launch_fb_points(desc_dev, ctx->fb_desc.d, n, max_pts, st);
    });
    return ts;
}

// What a push may ask of the raw images of a stream beyond "not null" (no HIP call): rows of at least w * bpp bytes, and
// 16-bit pixels on 2-byte boundaries.
static int px_check_images(const mskf_stream *s, const uint8_t *cam0, const uint8_t *cam1, long long pitch) {
    if (pitch < (long long)s->w * s->px.bpp) { mskf_set_error("image size differs from the calibration"); return MSKF_ERR_INVALID; }
    if (s->px.cfg.format == PX_GRAY16 && ((((uintptr_t)cam0 | (uintptr_t)cam1) & 1) || (pitch & 1))) {
        mskf_set_error("input format: MSKF_PIX_GRAY16 images and their pitch must be 2-byte aligned");
        return MSKF_ERR_INVALID;
    }
    return MSKF_OK;
}

// The converting images of a push: their jobs, and the size of the largest of them.
struct PxLaunch {
    int n = 0, max_w = 0, max_h = 0;
    void add(PxJob *jobs, const mskf_stream *s, const uint8_t *src, uint8_t *dst) {
        PxJob &j = jobs[n++];
        j.src = src; j.dst = dst; j.pitch = (long long)s->w * s->px.bpp;
        j.w = s->w; j.h = s->h; j.format = s->px.cfg.format; j.shift = s->px.cfg.shift;
        max_w = std::max(max_w, j.w); max_h = std::max(max_h, j.h);
    }
};

// A push in the manner of the update batch: plan_push looks at the whole batch and decides everything, touching nothing (no
// HIP call; every refusal of a push comes from here); push_accepted then waits for the staging, grows the arenas, commits
// the streams' and the context's fields and enqueues.
struct PushPlan {
    size_t cell_bytes = 0;            // the batch's slice of cell_arena (stream i's slice follows stream i - 1's)
    int max_w = 0, max_h = 0;
    long long px_pyr = 0, px_det = 0; // timing units: output pixels of the levels 1 .. 3 of both cameras, pixels of cam0 level 0
};
// (mskf_fe_push_stereo with padded rows enqueues its 2-D copies into the stream's own planes, or its raw staging, BEFORE it comes
// here: a refusal added to this function must also be looked at there, ahead of those copies, as px_check_images and
// mskf_refuse_if_owned are for a converting stream.)
static int plan_push(const mskf_ctx *ctx, int n, const mskf_stream *const *streams, const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, PushPlan &P) {
    if (!ctx || n <= 0 || !streams || !cam0 || !cam1) return MSKF_ERR_INVALID;
    // the pinned staging of a pending batch (descriptors, pyramid jobs, the cell arena) may still be in flight
    if (const int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_FE)) return rc;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        if (!s || s->ctx != ctx || !cam0[i] || !cam1[i]) return MSKF_ERR_INVALID;
        // on_device 3: level 0 already sits in the stream's own planes (mskf_fe_push_stereo with padded rows)
        // (a converting stream: the raw rasters already sit in its raw staging)
        if (on_device == 3 && (s->px.raw ? (cam0[i] != s->px.raw || cam1[i] != s->px.raw + px_raw_bytes(s))
                                         : (cam0[i] != s->pyr[s->i_curr0] || cam1[i] != s->pyr[s->i_curr1]))) return MSKF_ERR_INVALID;
        if (s->px.raw) { if (const int rc = px_check_images(s, cam0[i], cam1[i], (long long)s->w * s->px.bpp)) return rc; }
        P.cell_bytes += cell_key_bytes(s);
        P.max_w = std::max(P.max_w, s->w); P.max_h = std::max(P.max_h, s->h);
        for (int l = 1; l < MSKF_LEVELS; ++l) P.px_pyr += 2LL * s->lw[l] * s->lh[l];
        P.px_det += (long long)s->w * s->h;
    }
    return MSKF_OK;
}

// An accepted push (the context's device is current).  copy_cells = false: the per-cell maxima stay on the device (the
// bookkeeping kernel of a device frame reads them there).  The caller drains the stream if this fails (DrainOnError).
static int push_accepted(mskf_ctx *ctx, int n, mskf_stream *const *streams, const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device, bool copy_cells,
                         const PushPlan &P) {
    hipStream_t st = ctx->stream;
    int rc;
    // A push returns once its work is enqueued, and its copy kernel reads the pinned job / descriptor arrays when it runs: a
    // second push straight after the first (push, swap, push) must not overwrite them before that, or the first builds the
    // pyramid the SECOND one described.  Every public (copy_cells) push records cell_ev behind its last command and the next
    // one waits for it here.  A device-frame push records nothing: its staging is protected by the pending frame batch
    // (mskf_refuse_if_owned, and _end drains the stream), and after one this wait is on an older mark, already satisfied.
    if (ctx->cell_mark_recorded && (rc = mskf_wait_event(ctx, &ctx->cell_ev, false)) != MSKF_OK) return rc;
    if ((rc = ctx->jobs.ensure((size_t)n * 2)) != MSKF_OK || (rc = ctx->desc[0].ensure(n)) != MSKF_OK) return rc;
    // the streams that equalise their level 0 (mskf_fe_set_equalize): none by default, and then nothing below differs
    int n_eq = 0;
    for (int i = 0; i < n; ++i) n_eq += streams[i]->eq.cfg.mode != EQ_OFF ? 2 : 0;
    if (n_eq && (rc = ctx->eq_jobs.ensure((size_t)n_eq)) != MSKF_OK) return rc;
    // ... and the streams that convert their raw images (mskf_fe_set_input_format): the same holds
    int n_px = 0;
    for (int i = 0; i < n; ++i) n_px += streams[i]->px.raw ? 2 : 0;
    if (n_px && (rc = ctx->px_jobs.ensure((size_t)n_px)) != MSKF_OK) return rc;
    // ... and the streams that track over more than four levels (mskf_fe_set_lk_levels): the same holds
    int n_deep = 0;
    for (int i = 0; i < n; ++i) n_deep += streams[i]->deep.any() ? 2 : 0;
    if (n_deep && (rc = ctx->deep_jobs.ensure((size_t)n_deep)) != MSKF_OK) return rc;
    // ... and the streams with a cam0 mask (mskf_fe_set_mask): the same holds
    MskfCopy mask_cp{};
    bool masked = false;
    if ((rc = stage_masks(ctx, 0, n, streams, true, &mask_cp, &masked)) != MSKF_OK) return rc;
    if (P.cell_bytes > ctx->cell_arena.cap) { if ((rc = ctx->cell_arena.ensure(P.cell_bytes)) != MSKF_OK) return rc; ctx->cell_keys_dirty = true; }
    // ---- commit: the streams belong to this push from here on
    ++ctx->push_gen;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        s->cell_off = off; off += cell_key_bytes(s);
        s->push_gen = ctx->push_gen;
        // on_device 2: borrowed device images, level 0 is read in place (caller keeps them valid and unchanged until the
        // second-next push of this stream: the previous frame's cam0 is the LK template of the next frame)
        // (an equalising stream writes the equalised image into its own plane: nothing stays borrowed)
        // (nor with a converting stream: the converted image is written into its own plane)
        const bool borrow = on_device == 2 && s->eq.cfg.mode == EQ_OFF && !s->px.raw;
        s->lvl0[s->i_curr0] = borrow ? cam0[i] : nullptr;
        s->lvl0[s->i_curr1] = borrow ? cam1[i] : nullptr;
        s->has_curr = true;
        s->held[s->i_curr0] = s->held[s->i_curr1] = true;
    }
    // ---- enqueue: level 0 of both cameras unless it is borrowed or already there, then the levels 1 .. 3 of both cameras of
    // every stream in ONE launch (k_pyr_down3), its jobs staged together with the detector's descriptors
    static_assert(MSKF_LEVELS == 4, "k_pyr_down3 builds exactly the levels 1, 2, 3");
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    EqLaunch eql;
    PxLaunch pxl;
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        const uint8_t *const img[2] = {cam0[i], cam1[i]};
        const bool eq = s->eq.cfg.mode != EQ_OFF;
        // a converting stream reads a device image where the caller has it (on_device 1 and 2 alike), a host image from its raw
        // staging, and writes its own plane: what follows (the equalisation included) finds level 0 there
        const bool cv = s->px.raw != nullptr;
        // an equalising stream reads a device image where the caller has it (on_device 1 and 2 alike) and writes its own plane
        const bool eq_from_caller = eq && !cv && (on_device == 1 || on_device == 2);
        for (int c = 0; c < 2; ++c) {
            const int pi = pyr_of_role(s, 1 + c);
            uint8_t *base = s->pyr[pi];
            if (cv) {
                const uint8_t *raw = img[c];
                if (on_device == 0 || on_device == 3) {
                    uint8_t *stage = s->px.raw + c * px_raw_bytes(s);
                    if (on_device == 0) MSKF_HIPCHK(hipMemcpyAsync(stage, img[c], px_raw_bytes(s), hipMemcpyHostToDevice, st));
                    raw = stage;
                }
                pxl.add(ctx->px_jobs.h, s, raw, base + s->lvl_off[0]);
            } else if (on_device != 2 && on_device != 3 && !eq_from_caller) {
                MSKF_HIPCHK(hipMemcpyAsync(base, img[c], (size_t)s->w * s->h, kind, st));
            }
            if (eq) eql.add(ctx->eq_jobs.h, s, c, eq_from_caller ? img[c] : base, base + s->lvl_off[0]);
            Pyr3Job &j = ctx->jobs.h[2 * (size_t)i + c];
            j.src = level0(s, pi);
            j.d1 = base + s->lvl_off[1]; j.d2 = base + s->lvl_off[2]; j.d3 = base + s->lvl_off[3];
            j.w0 = s->lw[0]; j.h0 = s->lh[0];
        }
        fill_fe_desc(s, ctx->desc[0].h[i]);
    }
    MskfCopy cp[5] = {{ctx->jobs.d, ctx->jobs.h, sizeof(Pyr3Job) * 2 * (size_t)n}, {ctx->desc[0].d, ctx->desc[0].h, sizeof(FeStreamDev) * (size_t)n}};
    int n_cp = 2;
    if (masked) cp[n_cp++] = mask_cp;
    if (eql.n) cp[n_cp++] = {ctx->eq_jobs.d, ctx->eq_jobs.h, sizeof(EqJob) * (size_t)eql.n};
    if (pxl.n) cp[n_cp++] = {ctx->px_jobs.d, ctx->px_jobs.h, sizeof(PxJob) * (size_t)pxl.n};
    if ((rc = mskf_copy_async(ctx, cp, n_cp)) != MSKF_OK) return rc;
    // raw images -> level 0 (fe_pixfmt.h): untimed, there is no MSKF_K_* kind for it
    if (pxl.n) fe_launch_px_convert(ctx->px_jobs.d, pxl.n, pxl.max_w, pxl.max_h, st);
    // histogram, LUT, apply (fe_equalize.h): untimed, there is no MSKF_K_* kind for them
    if (eql.n) fe_launch_equalize(ctx->eq_jobs.d, eql.n, eql.max_units, eql.any_global, eql.max_regions, eql.splits, st);
    int ts = mskf_t_begin(ctx, MSKF_K_PYR);
    fe_launch_pyr_down3(ctx->jobs.d, 2 * n, P.max_w, P.max_h, st);
    mskf_t_end(ctx, ts, P.px_pyr);
    if (n_deep) {
        // the levels 4 and up of the deep streams' images, from the level 3 that launch has just written (fe_deep.hip)
        long long px_deep = 0;
        int k = 0;
        for (int i = 0; i < n; ++i) {
            const mskf_stream *s = streams[i];
            if (!s->deep.any()) continue;
            for (int c = 0; c < 2; ++c) {
                const int pi = pyr_of_role(s, 1 + c);
                DeepPyrJob &j = ctx->deep_jobs.h[k++];
                std::memset(&j, 0, sizeof(j));
                j.src = s->pyr[pi] + s->lvl_off[MSKF_LEVELS - 1];
                j.w = s->lw[MSKF_LEVELS - 1]; j.h = s->lh[MSKF_LEVELS - 1]; j.levels = s->deep.levels;
                for (int l = MSKF_LEVELS; l < s->deep.levels; ++l) {
                    j.dst[l - MSKF_LEVELS] = s->deep.level(pi, l);
                    px_deep += (long long)s->deep.w[l - MSKF_LEVELS] * s->deep.h[l - MSKF_LEVELS];
                }
            }
        }
        const MskfCopy dcp = {ctx->deep_jobs.d, ctx->deep_jobs.h, sizeof(DeepPyrJob) * (size_t)n_deep};
        if ((rc = mskf_copy_async(ctx, &dcp, 1)) != MSKF_OK) return rc;
        ts = mskf_t_begin(ctx, MSKF_K_PYR_DEEP);
        fe_launch_pyr_down_deep(ctx->deep_jobs.d, n_deep, st);
        mskf_t_end(ctx, ts, px_deep);
    }
    // detector per-cell maxima on cam0 level 0.  The keys carry the push generation in their top byte: a newer push wins every
    // atomicMax, so the key array is cleared only when it is fresh or the 8-bit generation wraps (not once per frame)
    const unsigned int gen = push_gen_tag(ctx->push_gen);
    if (ctx->cell_keys_dirty || gen == 1U) {
        MSKF_HIPCHK(hipMemsetAsync(ctx->cell_arena.d, 0, ctx->cell_arena.cap, st));
        ctx->cell_keys_dirty = false;
    }
    ts = mskf_t_begin(ctx, MSKF_K_DETECT);
    if (masked) fe_launch_detect_masked(ctx->desc[0].d, ctx->mask_desc[0].d, n, P.max_w, P.max_h, gen, st);      // the other instantiation of the same kernel
    else fe_launch_detect(ctx->desc[0].d, n, P.max_w, P.max_h, gen, st);
    mskf_t_end(ctx, ts, P.px_det);
    if (copy_cells) {
        const MskfCopy out = {ctx->cell_arena.h, ctx->cell_arena.d, P.cell_bytes};
        if ((rc = mskf_copy_async(ctx, &out, 1)) != MSKF_OK || (rc = mskf_wait_event(ctx, &ctx->cell_ev, true)) != MSKF_OK) return rc;
        ctx->cell_mark_recorded = true;
    }
    MSKF_HIPCHK(hipGetLastError());
    return MSKF_OK;
}

extern "C" int mskf_fe_push_stereo_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const uint8_t *const *cam0, const uint8_t *const *cam1, int on_device) {
    PushPlan P;
    int rc;
    if ((rc = plan_push(ctx, n, streams, cam0, cam1, on_device, P)) != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    DrainOnError drain{ctx->stream, true};
    if ((rc = push_accepted(ctx, n, streams, cam0, cam1, on_device, true, P)) != MSKF_OK) return rc;
    drain.armed = false;
    return MSKF_OK;
}

extern "C" int mskf_fe_push_stereo(mskf_stream *s, const uint8_t *cam0, const uint8_t *cam1, int width, int height, int pitch,
                                   double time_stamp) {
    if (!s || !cam0 || !cam1) return MSKF_ERR_INVALID;
    if (width != s->w || height != s->h || pitch < width * s->px.bpp) { mskf_set_error("image size differs from the calibration"); return MSKF_ERR_INVALID; }
    const uint8_t *a[1] = {cam0}, *b[1] = {cam1};
    mskf_stream *ss[1] = {s};
    if (s->px.raw && pitch != width * s->px.bpp) {
        // padded rows of a converting stream: the same, into its raw staging; everything a push can be refused for is looked at
        // before the copies are enqueued
        int rc;
        if ((rc = px_check_images(s, cam0, cam1, pitch)) != MSKF_OK || (rc = mskf_refuse_if_owned(s->ctx, MSKF_ARENAS_FE)) != MSKF_OK) return rc;
        s->time_stamp = time_stamp;
        const size_t row = (size_t)width * s->px.bpp;
        uint8_t *stage[2] = {s->px.raw, s->px.raw + px_raw_bytes(s)};
        MSKF_HIPCHK(hipSetDevice(s->ctx->device));
        MSKF_HIPCHK(hipMemcpy2DAsync(stage[0], row, cam0, pitch, row, height, hipMemcpyHostToDevice, s->ctx->stream));
        MSKF_HIPCHK(hipMemcpy2DAsync(stage[1], row, cam1, pitch, row, height, hipMemcpyHostToDevice, s->ctx->stream));
        a[0] = stage[0]; b[0] = stage[1];
        return mskf_fe_push_stereo_batch(s->ctx, 1, ss, a, b, 3);
    }
    s->time_stamp = time_stamp;
    if (pitch != width * s->px.bpp) {
        // padded rows: 2D copies straight into the stream's own level-0 planes (dense, pitch = width), then the batch
        // path with "level 0 already resident" (on_device = 3): no temporary allocation, nothing to free or leak
        MSKF_HIPCHK(hipSetDevice(s->ctx->device));
        MSKF_HIPCHK(hipMemcpy2DAsync(s->pyr[s->i_curr0], width, cam0, pitch, width, height, hipMemcpyHostToDevice, s->ctx->stream));
        MSKF_HIPCHK(hipMemcpy2DAsync(s->pyr[s->i_curr1], width, cam1, pitch, width, height, hipMemcpyHostToDevice, s->ctx->stream));
        a[0] = s->pyr[s->i_curr0]; b[0] = s->pyr[s->i_curr1];
    }
    return mskf_fe_push_stereo_batch(s->ctx, 1, ss, a, b, pitch != width * s->px.bpp ? 3 : 0);
}

extern "C" int mskf_fe_push_stereo_device(mskf_stream *s, const uint8_t *d_cam0, const uint8_t *d_cam1, int width, int height,
                                          double time_stamp) {
    if (!s || !d_cam0 || !d_cam1) return MSKF_ERR_INVALID;
    if (width != s->w || height != s->h) return MSKF_ERR_INVALID;
    s->time_stamp = time_stamp;
    const uint8_t *a[1] = {d_cam0}, *b[1] = {d_cam1};
    mskf_stream *ss[1] = {s};
    return mskf_fe_push_stereo_batch(s->ctx, 1, ss, a, b, 1);
}

// keys -> corners: gen (8) | score (24) | ~order (32), order = row-major position inside the cell; a key of another
// generation (an older push, or 0) means no corner in this one
static inline long long score_of_key(unsigned long long k, unsigned int gen) { return (k >> 56) == gen ? (long long)((k >> 32) & 0xFFFFFFULL) : 0LL; }
static inline void corner_of_key(const mskf_stream *s, int cell, unsigned long long k, mskf_corner &o) {
    o.cell = cell;
    const long long sc = score_of_key(k, push_gen_tag(s->push_gen));
    if (sc == 0) { o.x = 0.f; o.y = 0.f; o.score = 0; return; }
    const int cols = s->fe.det_cols, cw = s->det_cw, ch = s->det_ch;
    const unsigned int order = 0xFFFFFFFFu - (unsigned int)(k & 0xFFFFFFFFULL);
    const int cy = cell / cols, cx = cell - cy * cols;
    o.score = (int)sc;
    o.y = (float)(cy * ch + (int)(order / (unsigned)cw));
    o.x = (float)(cx * cw + (int)(order % (unsigned)cw));
}

static int cell_keys_ready(mskf_stream *s) {
    if (!s->has_curr) { mskf_set_error("no stereo pair pushed yet"); return MSKF_ERR_INVALID; }
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    if (s->push_gen != s->ctx->push_gen) { mskf_set_error("cell maxima are stale: another push happened on this context"); return MSKF_ERR_INVALID; }
    // wait for the copy of this push's maxima only (not the whole stream: on a shared stream another context may have
    // queued later work); no ctx mutation here: callable concurrently for different streams
    return mskf_wait_event(s->ctx, &s->ctx->cell_ev, false);
}

extern "C" int mskf_fe_set_detect_floor(mskf_stream *s, int min_score) {
    if (!s || min_score < 0 || min_score >= (1 << 24)) return MSKF_ERR_INVALID;
    s->det_floor = min_score;           // takes effect with the next push
    return MSKF_OK;
}

extern "C" int mskf_fe_get_cell_maxima(mskf_stream *s, mskf_corner *out, int capacity, int *n_out) {
    if (!s || !out || !n_out) return MSKF_ERR_INVALID;
    const int n = s->fe.det_rows * s->fe.det_cols;
    if (capacity < n) return MSKF_ERR_CAPACITY;
    const int rc = cell_keys_ready(s);
    if (rc != MSKF_OK) return rc;
    const unsigned long long *keys = (const unsigned long long *)(s->ctx->cell_arena.h + s->cell_off);
    for (int cell = 0; cell < n; ++cell) corner_of_key(s, cell, keys[cell], out[cell]);
    *n_out = n;
    return MSKF_OK;
}

extern "C" int mskf_fe_get_cell_candidates(mskf_stream *s, int min_score, mskf_corner *out, int capacity, int *n_out) {
    if (!s || !out || !n_out) return MSKF_ERR_INVALID;
    const int n = s->fe.det_rows * s->fe.det_cols;
    if (min_score < s->det_floor) { mskf_set_error("min_score is below the stream's detector floor (mskf_fe_set_detect_floor)"); return MSKF_ERR_INVALID; }
    const int rc = cell_keys_ready(s);
    if (rc != MSKF_OK) return rc;
    const unsigned long long *keys = (const unsigned long long *)(s->ctx->cell_arena.h + s->cell_off);
    const unsigned int gen = push_gen_tag(s->push_gen);
    int m = 0;
    for (int cell = 0; cell < n; ++cell) {
        const unsigned long long k = keys[cell];
        if (score_of_key(k, gen) <= (long long)min_score) continue;       // also skips empty cells (no key of this generation)
        if (m >= capacity) return MSKF_ERR_CAPACITY;
        corner_of_key(s, cell, k, out[m++]);
    }
    *n_out = m;
    return MSKF_OK;
}

extern "C" int mskf_fe_track_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_fe_track_args *args) {
    const int rc = mskf_fe_track_batch_begin(ctx, n, streams, args);
    return rc != MSKF_OK ? rc : mskf_fe_track_batch_end(ctx);
}

// One stream's result block of a track batch in trk_out, for np points: out0, out1, und0, und1, status.  Returns its size.
struct TrackOut { mskf_point2f *out0, *out1, *und0, *und1; uint8_t *status; };
static size_t track_out_block(char *base, size_t np, TrackOut &o) {       // (a null base only asks for the size)
    const uintptr_t b = (uintptr_t)base;
    const size_t pts = sizeof(mskf_point2f) * np;
    o.out0 = (mskf_point2f *)b; o.out1 = (mskf_point2f *)(b + pts); o.und0 = (mskf_point2f *)(b + 2 * pts); o.und1 = (mskf_point2f *)(b + 3 * pts);
    o.status = (uint8_t *)(b + 4 * pts);
    return round_up(4 * pts + np, 64);
}

extern "C" int mskf_fe_track_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_fe_track_args *args) {
    if (!ctx || n <= 0 || !streams || !args) return MSKF_ERR_INVALID;
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_FE);
    if (rc != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    const auto t_h0 = std::chrono::steady_clock::now();
    rc = ctx->desc[1].ensure(n);
    if (rc != MSKF_OK) return rc;
    int max_pts = 0;
    size_t in_bytes = 0, out_bytes = 0;
    std::vector<size_t> &in_off = ctx->pend_trk.in_off, &out_off = ctx->pend_trk.out_off;      // (no batch is pending: nobody reads them)
    in_off.resize(n); out_off.resize(n);
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        const mskf_fe_track_args &a = args[i];
        if (!s || s->ctx != ctx || a.n < 0) return MSKF_ERR_INVALID;
        if (a.n > s->pt_cap) { mskf_set_error("too many points for this stream"); return MSKF_ERR_CAPACITY; }
        if (a.n > 0 && (!a.in_pts || !a.out0 || !a.out1 || !a.und0 || !a.und1 || !a.status)) return MSKF_ERR_INVALID;
        if (!s->has_curr) { mskf_set_error("no stereo pair pushed yet"); return MSKF_ERR_INVALID; }
        in_off[i] = in_bytes; out_off[i] = out_bytes;
        TrackOut o;
        in_bytes += round_up(sizeof(mskf_point2f) * (size_t)a.n, 64);
        out_bytes += track_out_block(nullptr, (size_t)a.n, o);
        max_pts = std::max(max_pts, a.n);
    }
    if (max_pts <= 0) return MSKF_OK;      // nothing to track: no batch pending, _end is a no-op
    if ((rc = ctx->trk_in.ensure(in_bytes)) != MSKF_OK || (rc = ctx->trk_out.ensure(out_bytes)) != MSKF_OK) return rc;
    TrackPass pass;
    if ((rc = plan_track_pass(ctx, n, streams, pass)) != MSKF_OK) return rc;
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        const mskf_fe_track_args &a = args[i];
        const size_t np = (size_t)a.n;
        FeStreamDev &d = ctx->desc[1].h[i];
        fill_fe_desc(s, d);
        d.n_pts = a.n;
        d.do_temporal = a.do_temporal;
        std::memcpy(d.Hpred, a.Hpred, sizeof(d.Hpred));
        if (np) std::memcpy(ctx->trk_in.h + in_off[i], a.in_pts, sizeof(mskf_point2f) * np);
        d.in_pts = (const mskf_point2f *)(ctx->trk_in.d + in_off[i]);
        TrackOut o;
        track_out_block(ctx->trk_out.d + out_off[i], np, o);
        d.out0 = o.out0; d.out1 = o.out1; d.und0 = o.und0; d.und1 = o.und1; d.status = o.status;
    }
    // one list: the batch's own segments, then the pass's (mskf_copy_async splits it at MSKF_COPY_SEGS)
    MskfCopy cp[2 + TrackPass::kMaxSegs] = {{ctx->trk_in.d, ctx->trk_in.h, in_bytes}, {ctx->desc[1].d, ctx->desc[1].h, sizeof(FeStreamDev) * (size_t)n}};
    const int n_cp = (int)(std::copy(pass.seg, pass.seg + pass.n_seg, cp + 2) - cp);
    mskf_ctx::PendingTrack &T = ctx->pend_trk;
    T.n = n; T.args = args;
    rc = mskf_enqueue_staged(ctx, T, cp, n_cp, [&] { T.ts = run_track_pass(ctx, pass, ctx->desc[1].d, n, max_pts); },
                             MskfCopy{ctx->trk_out.h, ctx->trk_out.d, out_bytes});
    if (rc != MSKF_OK) return rc;
    if (ctx->t_gate) ctx->host_s[2] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h0).count();
    return MSKF_OK;
}

// Wait for the batch started by mskf_fe_track_batch_begin and copy its results into the args given there (which, like
// their output arrays, must still be valid).  No-op when nothing is pending.
extern "C" int mskf_fe_track_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    if (!ctx->pend_trk.active) return MSKF_OK;
    const int rc = mskf_batch_finish(ctx, ctx->pend_trk);
    if (rc != MSKF_OK) return rc;
    const mskf_ctx::PendingTrack &T = ctx->pend_trk;
    const auto t_h1 = std::chrono::steady_clock::now();
    long long tracks_t = 0, tracks_s = 0;
    for (int i = 0; i < T.n; ++i) {
        const mskf_fe_track_args &a = T.args[i];
        const size_t np = (size_t)a.n;
        if (!np) continue;
        TrackOut o;
        track_out_block(ctx->trk_out.h + T.out_off[i], np, o);
        const size_t pts = sizeof(mskf_point2f) * np;
        std::memcpy(a.out0, o.out0, pts); std::memcpy(a.out1, o.out1, pts); std::memcpy(a.und0, o.und0, pts); std::memcpy(a.und1, o.und1, pts);
        std::memcpy(a.status, o.status, np);
        // units of an LK launch = point tracks it executed: temporal (n of the temporal streams), stereo (the points that
        // passed the temporal gate, or all n of a stereo-only stream)
        if (a.do_temporal) { tracks_t += (long long)np; for (size_t k = 0; k < np; ++k) tracks_s += (a.status[k] & 1); }
        else tracks_s += (long long)np;
    }
    mskf_t_set_units(ctx, T.ts, MSKF_K_LK, tracks_t + tracks_s);      // point tracks of the launch: temporal + stereo
    mskf_t_collect(ctx);
    if (ctx->t_gate) ctx->host_s[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h1).count();
    return MSKF_OK;
}

extern "C" int mskf_fe_track(mskf_stream *s, const mskf_fe_track_args *args) {
    if (!s || !args) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    return mskf_fe_track_batch(s->ctx, 1, ss, args);
}

extern "C" int mskf_fe_swap(mskf_stream *s) {
    if (!s) return MSKF_ERR_INVALID;
    std::swap(s->i_prev0, s->i_curr0);
    s->has_curr = false;
    return MSKF_OK;
}

// ------------------------------------------------------------------------------------------ a whole frame on the device
extern "C" int mskf_fe_grid_capacity(mskf_stream *s) { return s ? s->book.dev.cap : 0; }

static int refuse_host_books() {
    mskf_set_error("this stream keeps its books on the host (grid_min / grid_max above the device limit)");
    return MSKF_ERR_UNSUPPORTED;
}

extern "C" int mskf_fe_set_grid(mskf_stream *s, int n, const uint64_t *id, const int32_t *lifetime, const mskf_point2f *cam0, const mskf_point2f *cam1,
                                const mskf_point2f *und0, const mskf_point2f *und1, uint64_t next_feature_id, const int32_t tracking_counters[3],
                                uint64_t ransac_draws) {
    if (!s || n < 0 || (n && (!id || !lifetime || !cam0 || !cam1 || !und0 || !und1))) return MSKF_ERR_INVALID;
    mskf_stream::Book &K = s->book;
    if (!K.dev.cap) return refuse_host_books();
    if (n > K.dev.cap) return MSKF_ERR_CAPACITY;
    mskf_ctx *ctx = s->ctx;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MSKF_HIPCHK(hipStreamSynchronize(st));      // (also: the previous set_grid's copy has read grid_in)
    // the seven arrays through the context's pinned grid_in, one staging copy
    const FeGridArr &G = K.grid[K.parity];
    const size_t n8 = round_up(8 * (size_t)n, 64), n4 = round_up(4 * (size_t)n, 64);
    const size_t o_st = 5 * n8 + n4;
    const int rc = ctx->grid_in.ensure(o_st + sizeof(FeBookState));
    if (rc != MSKF_OK) return rc;
    char *hs = ctx->grid_in.h;
    if (n) {
        std::memcpy(hs, id, 8 * (size_t)n);
        std::memcpy(hs + n8, lifetime, 4 * (size_t)n);
        std::memcpy(hs + n8 + n4, cam0, 8 * (size_t)n);
        std::memcpy(hs + 2 * n8 + n4, cam1, 8 * (size_t)n);
        std::memcpy(hs + 3 * n8 + n4, und0, 8 * (size_t)n);
        std::memcpy(hs + 4 * n8 + n4, und1, 8 * (size_t)n);
    }
    FeBookState &h = *(FeBookState *)(hs + o_st);
    std::memset(&h, 0, sizeof(h));
    h.next_id = next_feature_id; h.n_prev = n; h.n_curr = n;
    h.ransac_draws = ransac_draws;
    if (tracking_counters) { h.after_tracking = tracking_counters[0]; h.after_matching = tracking_counters[1]; h.after_ransac = tracking_counters[2]; }
    const MskfCopy cp[7] = {{G.id, hs, 8 * (size_t)n}, {G.lifetime, hs + n8, 4 * (size_t)n}, {G.cam0, hs + n8 + n4, 8 * (size_t)n},
                            {G.cam1, hs + 2 * n8 + n4, 8 * (size_t)n}, {G.und0, hs + 3 * n8 + n4, 8 * (size_t)n},
                            {G.und1, hs + 4 * n8 + n4, 8 * (size_t)n}, {K.dev.st, hs + o_st, sizeof(FeBookState)}};
    const int crc = mskf_copy_async(ctx, cp, 7);
    MSKF_HIPCHK(hipStreamSynchronize(st));
    if (crc != MSKF_OK) return crc;
    K.n_prev = n; K.n_cand_last = -1; K.grid_set = true;
    return MSKF_OK;
}

extern "C" int mskf_fe_frame_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, const uint8_t *const *cam0, const uint8_t *const *cam1,
                                         int on_device, mskf_fe_frame_args *args) {
    // ---- plan: the push's checks (arguments, no pending batch, streams, images), then the frame's own; nothing is touched
    // before both have passed
    PushPlan P;
    int rc;
    if (!args) return MSKF_ERR_INVALID;
    if ((rc = plan_push(ctx, n, streams, cam0, cam1, on_device, P)) != MSKF_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const mskf_stream::Book &K = streams[i]->book;
        if (!K.dev.cap) return refuse_host_books();
        if (!K.grid_set) { mskf_set_error("no grid on the device yet: the first frame goes through mskf_fe_track + mskf_fe_set_grid"); return MSKF_ERR_INVALID; }
        const mskf_fe_frame_args &a = args[i];
        if (a.capacity < K.dev.cap || !a.id || !a.lifetime || !a.cam0 || !a.cam1 || !a.und0 || !a.und1) return MSKF_ERR_INVALID;
    }
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const auto t_h0 = std::chrono::steady_clock::now();
    // ---- accepted: a failure from here on drains the stream before it is reported
    DrainOnError drain{st, true};        // (the push enqueues the images, the pyramids and the detector)
    if ((rc = push_accepted(ctx, n, streams, cam0, cam1, on_device, false, P)) != MSKF_OK) return rc;
    if ((rc = ctx->desc[1].ensure(n)) != MSKF_OK || (rc = ctx->desc[2].ensure(n)) != MSKF_OK || (rc = ctx->book_desc.ensure(n)) != MSKF_OK) return rc;
    std::vector<size_t> &out_off = ctx->pend_frame.out_off;
    out_off.resize(n);
    size_t out_bytes = 0, scratch_bytes = 0;
    int max_prev = 0, max_cand_est = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_stream::Book &K = streams[i]->book;
        const FeBookDev &D = K.dev;
        FeExport x;
        out_off[i] = out_bytes;
        out_bytes += round_up(fe_book_export(nullptr, D.cap, x), 256);
        scratch_bytes = std::max(scratch_bytes, 4 * fe_book_scratch_ints(D.cap, D.cand_cap, D.det_cap, D.n_codes, D.det_cap));
        max_prev = std::max(max_prev, K.n_prev);
        // candidates are counted on the device: the launch is sized from the last frame's count, a block takes several point
        // groups if there are more this time
        const int est = K.n_cand_last < 0 ? D.cand_cap / 2 : std::min(D.cand_cap, K.n_cand_last + K.n_cand_last / 2 + 32);
        max_cand_est = std::max(max_cand_est, est);
    }
    if ((rc = ctx->book_out.ensure(out_bytes)) != MSKF_OK) return rc;
    TrackPass pass;                         // (one plan serves both passes of the frame)
    if ((rc = plan_track_pass(ctx, n, streams, pass)) != MSKF_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        const mskf_stream::Book &K = s->book;
        const FeBookDev &D = K.dev;
        // first track call: the previous grid's cam0 points, temporal + stereo
        FeStreamDev &d1 = ctx->desc[1].h[i];
        fill_fe_desc(s, d1);
        d1.n_pts = K.n_prev; d1.n_pts_dev = nullptr; d1.do_temporal = 1;
        std::memcpy(d1.Hpred, args[i].Hpred, sizeof(d1.Hpred));
        d1.in_pts = K.grid[K.parity].cam0;
        d1.out0 = (mskf_point2f *)D.t_out0; d1.out1 = (mskf_point2f *)D.t_out1; d1.und0 = (mskf_point2f *)D.t_und0; d1.und1 = (mskf_point2f *)D.t_und1; d1.status = (uint8_t *)D.t_status;
        // second track call: the candidates fe_book1 leaves in the stream's list, stereo only
        FeStreamDev &d2 = ctx->desc[2].h[i];
        fill_fe_desc(s, d2);
        d2.n_pts = 0; d2.n_pts_dev = &D.st->n_cand; d2.do_temporal = 0;
        d2.Hpred[0] = d2.Hpred[4] = d2.Hpred[8] = 1.0;
        d2.in_pts = D.cand_pt;
        d2.out0 = (mskf_point2f *)D.c_out0; d2.out1 = (mskf_point2f *)D.c_out1; d2.und0 = (mskf_point2f *)D.c_und0; d2.und1 = (mskf_point2f *)D.c_und1; d2.status = (uint8_t *)D.c_status;
        // the books: the stream's constant descriptor plus what this frame brings
        FeBookDev &B = ctx->book_desc.h[i];
        B = D;
        B.gen = push_gen_tag(s->push_gen);
        std::memcpy(B.R_p_c, args[i].R_p_c, sizeof(B.R_p_c));
        B.prev = K.grid[K.parity]; B.curr = K.grid[K.parity ^ 1];
        B.cell_keys = (const unsigned long long *)(ctx->cell_arena.d + s->cell_off);
        FeExport x;
        fe_book_export(ctx->book_out.d + out_off[i], D.cap, x);
        B.x_info = x.info; B.x_id = x.id; B.x_lifetime = x.lifetime; B.x_cam0 = x.cam0; B.x_cam1 = x.cam1; B.x_und0 = x.und0; B.x_und1 = x.und1;
    }
    {
        // one list: the frame's own segments, then the pass's (mskf_copy_async splits it at MSKF_COPY_SEGS)
        MskfCopy cp[3 + TrackPass::kMaxSegs] = {{ctx->desc[1].d, ctx->desc[1].h, sizeof(FeStreamDev) * (size_t)n}, {ctx->desc[2].d, ctx->desc[2].h, sizeof(FeStreamDev) * (size_t)n},
                                                {ctx->book_desc.d, ctx->book_desc.h, sizeof(FeBookDev) * (size_t)n}};
        const int n_cp = (int)(std::copy(pass.seg, pass.seg + pass.n_seg, cp + 3) - cp);
        if ((rc = mskf_copy_async(ctx, cp, n_cp)) != MSKF_OK) return rc;
    }
    const int ts1 = run_track_pass(ctx, pass, ctx->desc[1].d, n, max_prev);
    int tb = mskf_t_begin(ctx, MSKF_K_FE_BOOK);
    fe_launch_book(ctx->book_desc.d, n, 0, scratch_bytes, st);
    mskf_t_end(ctx, tb, n);
    const int ts2 = run_track_pass(ctx, pass, ctx->desc[2].d, n, std::max(max_cand_est, 4));
    tb = mskf_t_begin(ctx, MSKF_K_FE_BOOK);
    fe_launch_book(ctx->book_desc.d, n, 1, scratch_bytes, st);
    mskf_t_end(ctx, tb, n);
    { const MskfCopy cp = {ctx->book_out.h, ctx->book_out.d, out_bytes}; if ((rc = mskf_copy_async(ctx, &cp, 1)) != MSKF_OK) return rc; }
    MSKF_HIPCHK(hipGetLastError());
    ctx->pend_frame.n = n; ctx->pend_frame.streams = streams; ctx->pend_frame.args = args;
    ctx->pend_frame.ts1 = ts1; ctx->pend_frame.ts2 = ts2;
    if ((rc = mskf_batch_arm(ctx, ctx->pend_frame)) != MSKF_OK) return rc;
    drain.armed = false;
    // state rotation (:192-200): the grid just built is the next frame's previous grid, curr cam0 becomes prev cam0
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        s->book.parity ^= 1;
        std::swap(s->i_prev0, s->i_curr0);
        s->has_curr = false;
    }
    if (ctx->t_gate) ctx->host_s[2] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h0).count();
    return MSKF_OK;
}

extern "C" int mskf_fe_frame_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingFrame &F = ctx->pend_frame;
    if (!F.active) return MSKF_OK;
    const int rc = mskf_batch_finish(ctx, F);
    if (rc != MSKF_OK) return rc;
    const auto t_h1 = std::chrono::steady_clock::now();
    long long tracks1 = 0, tracks2 = 0;
    bool overflow = false;
    for (int i = 0; i < F.n; ++i) {
        mskf_stream::Book &K = F.streams[i]->book;
        mskf_fe_frame_args &a = F.args[i];
        FeExport x;
        fe_book_export(ctx->book_out.h + F.out_off[i], K.dev.cap, x);
        const int *info = x.info;
        const int m = info[FX_N_CURR];
        if (m < 0 || m > K.dev.cap || info[FX_OVERFLOW]) { overflow = true; continue; }
        a.n = m; a.n_candidates = info[FX_N_CAND];
        a.before_tracking = info[FX_BEFORE_TRACKING]; a.after_tracking = info[FX_AFTER_TRACKING]; a.after_matching = info[FX_AFTER_MATCHING]; a.after_ransac = info[FX_AFTER_RANSAC];
        a.next_feature_id = (uint64_t)(unsigned int)info[FX_NEXT_ID_LO] | ((uint64_t)(unsigned int)info[FX_NEXT_ID_HI] << 32);
        a.n_new = info[FX_N_NEW];
        a.ransac_draws = (uint64_t)(unsigned int)info[FX_RANSAC_DRAWS_LO] | ((uint64_t)(unsigned int)info[FX_RANSAC_DRAWS_HI] << 32);
        const size_t pts = sizeof(mskf_point2f) * (size_t)m;
        std::memcpy(a.id, x.id, sizeof(*x.id) * (size_t)m); std::memcpy(a.lifetime, x.lifetime, sizeof(*x.lifetime) * (size_t)m);
        std::memcpy(a.cam0, x.cam0, pts); std::memcpy(a.cam1, x.cam1, pts); std::memcpy(a.und0, x.und0, pts); std::memcpy(a.und1, x.und1, pts);
        tracks1 += (long long)a.before_tracking + (a.before_tracking > 0 ? a.after_tracking : 0);
        tracks2 += a.n_candidates;
        K.n_prev = m; K.n_cand_last = a.n_candidates;
    }
    mskf_t_set_units(ctx, F.ts1, MSKF_K_LK, tracks1);
    mskf_t_set_units(ctx, F.ts2, MSKF_K_LK, tracks2);
    mskf_t_collect(ctx);
    if (ctx->t_gate) ctx->host_s[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h1).count();
    if (overflow) { mskf_set_error("device bookkeeping reported a capacity overflow"); return MSKF_ERR_CAPACITY; }
    return MSKF_OK;
}

extern "C" int mskf_fe_get_level(mskf_stream *s, int role, int level, uint8_t *out, int capacity, int *w, int *h) {
    if (!s || !out || role < 0 || role > 2 || level < 0 || level >= s->deep.levels) return MSKF_ERR_INVALID;      // (4 unless mskf_fe_set_lk_levels)
    const int idx = pyr_of_role(s, role);
    const bool hi = level >= MSKF_LEVELS;
    const int lw = hi ? s->deep.w[level - MSKF_LEVELS] : s->lw[level], lh = hi ? s->deep.h[level - MSKF_LEVELS] : s->lh[level];
    const size_t bytes = (size_t)lw * lh;
    if ((size_t)capacity < bytes) return MSKF_ERR_CAPACITY;
    MSKF_HIPCHK(hipSetDevice(s->ctx->device));
    MSKF_HIPCHK(hipStreamSynchronize(s->ctx->stream));
    const uint8_t *src = level == 0 ? level0(s, idx) : hi ? s->deep.level(idx, level) : s->pyr[idx] + s->lvl_off[level];
    MSKF_HIPCHK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    if (w) *w = lw;
    if (h) *h = lh;
    return MSKF_OK;
}
