// j2k_rate.cpp -- rate control of the MQ block coder behind the C ABI: the plan's band weights, the table-filling block encode, the allocation
// of a byte budget (kernels: t1.hip's PLANES instantiations, rate.hip).  include/j2kgfx.h has the contract, tests/rate_cases.py the definition.
#include <cmath>

#include "j2k_host.h"

using namespace j2k;

// ---- band weights: the synthesis energy gain of a sub-band ---------------------------------------------------------------------------------
// One level of the 1-D inverse transform as the reference's lifting steps without their integer rounding (dwt.go:122-147, 213-262), run on a
// line long enough that an impulse in its middle never meets the ends: the response to a low-pass and to a high-pass sample.
static std::vector<double> synth_response(int wavelet, bool high) {
    const int n = 64, half = n / 2;
    std::vector<double> d(n, 0.0);
    d[high ? 2 * (half / 2) + 1 : 2 * (half / 2)] = 1.0;             // already interleaved: even = low, odd = high
    auto lift = [&](int first, double c) {                           // d[i] -= c * (d[i-1] + d[i+1]) on the samples of one parity (interior only)
        for (int i = first ? 1 : 2; i < n - 1; i += 2) d[i] -= c * (d[i - 1] + d[i + 1]);
    };
    if (wavelet == W53) {
        lift(0, 0.25);
        lift(1, -0.5);
    } else {
        const double K = 1.230174104914001, KINV = 0.812893066115961;
        for (int i = 0; i < n; i++) d[i] *= (i & 1) ? KINV : K;
        lift(0, 0.443506852043971);
        lift(1, 0.882911075530934);
        lift(0, -0.052980118572961);
        lift(1, -1.586134342059924);
    }
    int a = 0, b = n - 1;
    while (a < b && d[a] == 0.0) a++;
    while (b > a && d[b] == 0.0) b--;
    return std::vector<double>(d.begin() + a, d.begin() + b + 1);
}
// one more synthesis level under a response: insert zeros, filter with the low-pass response
static std::vector<double> synth_deeper(const std::vector<double> &f, const std::vector<double> &g0) {
    std::vector<double> out(2 * f.size() - 1 + g0.size() - 1, 0.0);
    for (size_t i = 0; i < f.size(); i++)
        for (size_t k = 0; k < g0.size(); k++) out[2 * i + k] += f[i] * g0[k];
    return out;
}
static double energy(const std::vector<double> &f) { double e = 0; for (double v : f) e += v * v; return e; }

static void plan_default_rate_weights(j2k_plan *P) {
    const PlanSpec &S = P->spec;
    const int numRes = S.num_res_jobs > 0 ? S.num_res_jobs : 6;
    P->rate_weights.assign((size_t)S.C * numRes * 4, 1.0);
    if (!S.mallat) return;                                           // the windows of the other modes are not sub-bands: every weight 1
    const int L = numRes - 1;
    // 1-D gains of a low-pass / high-pass sample d levels down, d = 1 ... L (exact up to 16 levels; deeper ones continue at the last ratio)
    std::vector<double> EL(L + 1, 1.0), EH(L + 1, 1.0);
    const std::vector<double> g0 = synth_response(S.wavelet, false), g1 = synth_response(S.wavelet, true);
    std::vector<double> fl = g0, fh = g1;
    for (int d = 1; d <= L; d++) {
        if (d > 1 && d <= 16) { fl = synth_deeper(fl, g0); fh = synth_deeper(fh, g0); }
        if (d <= 16) { EL[d] = energy(fl); EH[d] = energy(fh); }
        else { EL[d] = EL[d - 1] * (EL[16] / EL[15]); EH[d] = EH[d - 1] * (EH[16] / EH[15]); }
    }
    for (int c = 0; c < S.C; c++)
        for (int r = 0; r < numRes; r++) {
            double *w = &P->rate_weights[((size_t)c * numRes + r) * 4];
            const int d = r == 0 ? L : L - r + 1;
            w[J2K_BAND_LL] = EL[d] * EL[d];
            w[J2K_BAND_HL] = w[J2K_BAND_LH] = EH[d] * EL[d];
            w[J2K_BAND_HH] = EH[d] * EH[d];
        }
}

static void plan_rate_weights(j2k_plan *P) {
    if (P->rate_weights.empty()) plan_default_rate_weights(P);
}

// what every rate call needs of its plan
int rate_check(j2k_plan *P, const char *who) {
    const PlanSpec &S = P->spec;
    const char *why = nullptr;
    if (S.coder != J2K_CODER_MQ) why = "needs the MQ coder (the HT coder's one pass has no planes to cut between)";
    else if (!S.closed_loop) why = "needs a closed-loop plan (only its packets can say where a block was cut)";
    else if (S.frame_h != S.H && !P->rate_per_frame) why = "a batch plan (frame_rows): not built";
    else if (P->raw_magref) why = "the plan codes in the raw-MagRef style (j2k_plan_set_raw_magref): a two-stream body cannot be cut at bit planes";
    else
        for (const j2k_block &b : P->blocks)
            if (b.w > 64 || b.h > 64) { why = "blocks above 64 x 64: not built"; break; }
    if (why) return fail(P->ctx, J2K_ERR_UNSUPPORTED, (std::string(who) + ": " + why).c_str());
    return J2K_OK;
}

// ---- batch plans: every frame allocated alone (tests/frame_rate_cases.py) -------------------------------------------------------
// Plan state in the idiom of j2k_plan_set_raw_magref: the rate calls read it, nothing below them does -- block coding, distortion, packets and
// readers already work per block or per tile.
extern "C" int j2k_plan_set_rate_per_frame(j2k_plan *P, int on) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_set_rate_per_frame: plan state cannot change while a graph is being captured");
    if (on != 0 && on != 1) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_set_rate_per_frame: on is 0 or 1");
    const PlanSpec &S = P->spec;
    if (on && S.frame_h > 0 && S.frame_h != S.H && P->tile_count != P->tiles_x * P->tiles_y)
        return fail(ctx, J2K_ERR_UNSUPPORTED, "j2k_plan_set_rate_per_frame: a shard of a batch plan (tile_first / tile_count): a frame may be partial");
    P->rate_per_frame = on != 0;
    return J2K_OK;
}
int rate_frames(const j2k_plan *P) {
    const PlanSpec &S = P->spec;
    return P->rate_per_frame && S.frame_h > 0 && S.frame_h < S.H ? S.H / S.frame_h : 1;
}
extern "C" int j2k_plan_rate_frames(const j2k_plan *P, int32_t *frames) {
    if (!P || !frames) return J2K_ERR_INVALID_ARG;
    *frames = rate_frames(P);
    return J2K_OK;
}

extern "C" int j2k_plan_get_rate_weights(j2k_plan *P, double *weights, size_t cap, size_t *count) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    plan_rate_weights(P);
    if (count) *count = P->rate_weights.size();
    if (!weights) return cap ? J2K_ERR_INVALID_ARG : J2K_OK;
    if (cap < P->rate_weights.size()) return J2K_ERR_CAPACITY;
    memcpy(weights, P->rate_weights.data(), P->rate_weights.size() * sizeof(double));
    return J2K_OK;
}

extern "C" int j2k_plan_set_rate_weights(j2k_plan *P, const double *weights, size_t count) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (P->ctx->capturing) return fail(P->ctx, J2K_ERR_INVALID_ARG, "capture: set the weights before j2k_ctx_capture_begin");
    plan_rate_weights(P);
    if (!weights) { plan_default_rate_weights(P); P->rate_wj_valid = false; return J2K_OK; }       // back to the default
    if (count != P->rate_weights.size()) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_plan_set_rate_weights: ncomp * num_resolutions * 4 weights");
    for (size_t i = 0; i < count; i++)
        if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_plan_set_rate_weights: weights are finite and >= 0");
    P->rate_weights.assign(weights, weights + count);
    P->rate_wj_valid = false;
    return J2K_OK;
}

extern "C" int j2k_plan_encode_blocks_planes(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps,
                                             uint32_t *d_rate, uint64_t *d_dist) {
    graph_note_plan(P);
    if (!P || !d_coeff || !d_slots || !d_lens || !d_numbps || !d_rate || !d_dist) return J2K_ERR_INVALID_ARG;
    int r = rate_check(P, "j2k_plan_encode_blocks_planes");
    if (r != J2K_OK) return r;
    r = plan_encode_blocks_impl(P, d_coeff, d_slots, d_lens, d_numbps, d_rate);
    if (r != J2K_OK) return r;
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, launch_rate_distortion(ctx->stream, P->d_bjobs, (int)P->blocks.size(), d_coeff, d_numbps, d_dist));
    return J2K_OK;
}

// ---- region of interest: the footprint of a rectangle counts roi_gain times in the distortion tables (tests/roi_cases.py) --------
int roi_check(j2k_plan *P, const j2k_rect *roi, int roi_gain, const char *who) {
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    const std::string w(who);
    if (!S.mallat) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": a region of interest needs a Mallat plan (the prefix layout has no spatial footprint below level 0)").c_str());
    if (P->tile_count != P->tiles_x * P->tiles_y) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": a region of interest on a shard plan (tile_first / tile_count)").c_str());
    if (rate_frames(P) > 1) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": a region of interest on a batch plan (the footprint tables know one frame)").c_str());
    if (!roi) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": no rectangle").c_str());
    if (roi->x0 < 0 || roi->y0 < 0 || roi->x0 >= roi->x1 || roi->y0 >= roi->y1 || roi->x1 > S.W || roi->y1 > S.H)
        return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": the rectangle is inverted, empty or outside the frame").c_str());
    if (roi_gain < 1 || roi_gain > 65535) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": roi_gain is 1 ... 65535").c_str());
    return J2K_OK;
}

extern "C" int j2k_plan_roi_windows(j2k_plan *P, const j2k_rect *roi, int32_t *d_win) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = rate_check(P, "j2k_plan_roi_windows");
    if (r == J2K_OK) r = roi_check(P, roi, 1, "j2k_plan_roi_windows");
    if (r != J2K_OK) return r;
    if (!d_win) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    if ((r = area_tables(P, false)) != J2K_OK) return r;
    HIPCHK(ctx, launch_roi_windows(ctx->stream, P->d_area_blocks, (int)P->blocks.size(), P->d_area_planes, roi->x0, roi->y0, roi->x1, roi->y1,
                                   P->spec.wavelet == W97 ? 2 : 1, d_win));
    return J2K_OK;
}

int plan_encode_blocks_planes_roi(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate, uint64_t *d_dist,
                                  const j2k_rect *roi, int roi_gain) {
    if (!roi) return j2k_plan_encode_blocks_planes(P, d_coeff, d_slots, d_lens, d_numbps, d_rate, d_dist);
    j2k_ctx *ctx = P->ctx;
    int r = area_tables(P, false);
    if (r == J2K_OK) r = plan_encode_blocks_impl(P, d_coeff, d_slots, d_lens, d_numbps, d_rate);
    if (r != J2K_OK) return r;
    HIPCHK(ctx, launch_rate_distortion_roi(ctx->stream, P->d_bjobs, (int)P->blocks.size(), d_coeff, d_numbps, P->d_area_blocks, P->d_area_planes, roi->x0, roi->y0,
                                           roi->x1, roi->y1, P->spec.wavelet == W97 ? 2 : 1, (uint32_t)roi_gain, d_dist));
    return J2K_OK;
}

extern "C" int j2k_plan_encode_blocks_planes_roi(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate,
                                                 uint64_t *d_dist, const j2k_rect *roi, int roi_gain) {
    graph_note_plan(P);
    if (!P || !d_coeff || !d_slots || !d_lens || !d_numbps || !d_rate || !d_dist) return J2K_ERR_INVALID_ARG;
    int r = rate_check(P, "j2k_plan_encode_blocks_planes_roi");
    if (r == J2K_OK) r = roi_check(P, roi, roi_gain, "j2k_plan_encode_blocks_planes_roi");
    if (r != J2K_OK) return r;
    return plan_encode_blocks_planes_roi(P, d_coeff, d_slots, d_lens, d_numbps, d_rate, d_dist, roi, roi_gain);
}

extern "C" int j2k_plan_rate_allocate(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, int64_t max_body_bytes,
                                      uint8_t *d_kept, uint64_t *d_chosen) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = rate_check(P, "j2k_plan_rate_allocate");
    if (r != J2K_OK) return r;
    if (max_body_bytes < 0) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_rate_allocate: a negative budget");
    EncodeRequest q;
    q.kind = EncodeRequest::BYTES;
    q.budgets[0] = (uint64_t)max_body_bytes;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, nullptr);
}

// The ONE allocation launch of a request (every stage call and the frame encoder end here): the weights, the workspace and -- on a batch plan with
// j2k_plan_set_rate_per_frame -- the frame ranges on the device, the per-frame values of a _frames call written on the stream, then the kernel its
// kind, layering and granularity select, F workgroups of it.  F = 1 passes no frame table: the launch is the one it has always been.
int rate_allocate_launch(j2k_plan *P, const EncodeRequest &q, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, uint8_t *d_kept,
                         uint64_t *d_chosen, double *d_achieved) {
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int r = rate_upload_weights(P);
    if (r != J2K_OK) return r;
    const int n = (int)P->blocks.size(), F = rate_frames(P);
    const RateFrame *frames = F > 1 ? P->d_rate_frames : nullptr;
    const uint64_t *fv = nullptr;
    if (q.per_frame && F > 1) {          // (F = 1: the callers have put the one value into budgets[0] / targets[0])
        HIPCHK(ctx, launch_rate_frame_values(ctx->stream, q.frame_values.data(), F, P->d_rate_fvals));
        fv = P->d_rate_fvals;
    }
    const bool quality = q.kind == EncodeRequest::DISTORTION;
    if (q.passes && quality)
        HIPCHK(ctx, launch_rate_allocate_quality_passes(ctx->stream, n, d_rate, d_dist, d_numbps, P->d_rate_wj, q.targets[0], P->d_rate_ws, d_kept, d_chosen, d_achieved, F, frames,
                                                        reinterpret_cast<const double *>(fv)));
    else if (q.passes)
        HIPCHK(ctx, launch_rate_allocate_passes(ctx->stream, n, d_rate, d_dist, d_numbps, P->d_rate_wj, q.budgets[0], P->d_rate_ws, d_kept, d_chosen, F, frames, fv));
    else if (quality)
        HIPCHK(ctx, launch_rate_allocate_quality(ctx->stream, n, d_rate, d_dist, d_numbps, P->d_rate_wj, q.targets, q.nlayers, P->d_rate_ws, d_kept, d_chosen, d_achieved, F, frames,
                                                 reinterpret_cast<const double *>(fv)));
    else if (q.layered)
        HIPCHK(ctx, launch_rate_allocate_layers(ctx->stream, n, d_rate, d_dist, d_numbps, P->d_rate_wj, q.budgets, q.nlayers, P->d_rate_ws, d_kept, d_chosen, F, frames));
    else
        HIPCHK(ctx, launch_rate_allocate(ctx->stream, n, d_rate, d_dist, d_numbps, P->d_rate_wj, q.budgets[0], P->d_rate_ws, d_kept, d_chosen, F, frames, fv));
    return J2K_OK;
}

// the vector of a _frames call -> the request: one entry per frame, each checked as the scalar it stands for (the entries belong to different
// frames: they need not fall or rise).  With F = 1 the one entry IS the scalar: budgets[0] / targets[0], and nothing per frame.
int frame_values_request(j2k_plan *P, const char *who, const int64_t *frame_bytes, const double *frame_targets, int nframes, EncodeRequest &q) {
    j2k_ctx *ctx = P->ctx;
    const std::string w(who);
    int r = rate_check(P, who);
    if (r != J2K_OK) return r;
    if ((frame_bytes != nullptr) == (frame_targets != nullptr)) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": exactly one of frame_bytes and frame_targets").c_str());
    const int F = rate_frames(P);
    if (nframes != F) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": one entry per frame of the plan (j2k_plan_rate_frames)").c_str());
    q = EncodeRequest();
    q.kind = frame_targets ? EncodeRequest::DISTORTION : EncodeRequest::BYTES;
    q.frame_values.resize((size_t)F);
    for (int f = 0; f < F; f++) {
        if (frame_bytes) {
            if (frame_bytes[f] < 0) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": a negative budget").c_str());
            q.frame_values[(size_t)f] = (uint64_t)frame_bytes[f];
        } else {
            if (!std::isfinite(frame_targets[f]) || frame_targets[f] < 0.0) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": a target is a finite distortion >= 0").c_str());
            memcpy(&q.frame_values[(size_t)f], &frame_targets[f], sizeof(double));
        }
    }
    if (frame_bytes) q.budgets[0] = (uint64_t)frame_bytes[0]; else q.targets[0] = frame_targets[0];
    q.per_frame = F > 1;
    return J2K_OK;
}

// j2k_plan_rate_allocate / _passes with a budget of its own for every frame of the batch
extern "C" int j2k_plan_rate_allocate_frames(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, const int64_t *frame_bytes, int nframes,
                                             int pass_cuts, uint8_t *d_kept, uint64_t *d_chosen) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen) return J2K_ERR_INVALID_ARG;
    if (!frame_bytes) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_plan_rate_allocate_frames: no budgets");
    EncodeRequest q;
    const int r = frame_values_request(P, "j2k_plan_rate_allocate_frames", frame_bytes, nullptr, nframes, q);
    if (r != J2K_OK) return r;
    q.passes = pass_cuts != 0;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, nullptr);
}
// j2k_plan_rate_allocate_quality (one layer) / _quality_passes with a target of its own for every frame
extern "C" int j2k_plan_rate_allocate_quality_frames(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, const double *frame_targets,
                                                     int nframes, int pass_cuts, uint8_t *d_kept, uint64_t *d_chosen, double *d_achieved) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen || !d_achieved) return J2K_ERR_INVALID_ARG;
    if (!frame_targets) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_plan_rate_allocate_quality_frames: no targets");
    EncodeRequest q;
    const int r = frame_values_request(P, "j2k_plan_rate_allocate_quality_frames", nullptr, frame_targets, nframes, q);
    if (r != J2K_OK) return r;
    q.passes = pass_cuts != 0;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, d_achieved);
}

// ---- the dual: a distortion target in the place of a byte budget (tests/quality_cases.py) ----------------------------------------
// T = N * peak^2 * q^2 / 10^(dB / 10): N samples, peak = 2^precision - 1, q = the plan's quality where it quantises (its coefficients are the
// transform times quality), else 1.  Host only.  N is the samples of ONE frame: on a batch plan with j2k_plan_set_rate_per_frame a target belongs
// to a frame (W * frame_rows * ncomp), on every other plan it is W * H * ncomp as ever.
extern "C" int j2k_plan_psnr_distortion(const j2k_plan *P, double db, double *T) {
    if (!P || !T || !std::isfinite(db)) return J2K_ERR_INVALID_ARG;
    const PlanSpec &S = P->spec;
    const double peak = (double)((1u << S.precision) - 1u), q = S.quant != Q_NONE ? (double)S.quality : 1.0;
    const double t = (double)S.W * (double)(S.H / rate_frames(P)) * (double)S.C * peak * peak * q * q / std::pow(10.0, db / 10.0);
    if (!std::isfinite(t)) return J2K_ERR_INVALID_ARG;
    *T = t;
    return J2K_OK;
}

// distortion targets: finite, none negative, none above the one before
int targets_check(j2k_ctx *ctx, const double *targets, int nlayers, const char *who) {
    if (!targets) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": no targets").c_str());
    for (int l = 0; l < nlayers; l++) {
        if (!std::isfinite(targets[l]) || targets[l] < 0.0) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": a target is a finite distortion >= 0").c_str());
        if (l && targets[l] > targets[l - 1]) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": the targets fall layer by layer -- none may be above the one before").c_str());
    }
    return J2K_OK;
}

extern "C" int j2k_plan_rate_allocate_quality(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, const double *targets, int nlayers,
                                              uint8_t *d_kept, uint64_t *d_chosen, double *d_achieved) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen || !d_achieved) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = rate_check(P, "j2k_plan_rate_allocate_quality");
    if (r != J2K_OK) return r;
    if (nlayers < 1 || nlayers > J2K_MAX_LAYERS) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_rate_allocate_quality: the layer count is 1 ... 32");
    r = targets_check(ctx, targets, nlayers, "j2k_plan_rate_allocate_quality");
    if (r != J2K_OK) return r;
    EncodeRequest q;
    q.kind = EncodeRequest::DISTORTION;
    q.nlayers = nlayers; q.layered = true;
    std::copy(targets, targets + nlayers, q.targets);
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, d_achieved);
}

int rate_upload_weights(j2k_plan *P) {
    j2k_ctx *ctx = P->ctx;
    const size_t n = P->blocks.size();
    if (!P->rate_wj_valid || !P->d_rate_ws) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: run the same calls once before j2k_ctx_capture_begin");
        plan_rate_weights(P);
        const int numRes = P->spec.num_res_jobs > 0 ? P->spec.num_res_jobs : 6;
        std::vector<double> wj(n + 1, 1.0);
        for (size_t j = 0; j < n; j++) {
            const j2k_block &b = P->blocks[j];
            wj[j] = P->rate_weights[((size_t)(b.plane % P->spec.C) * numRes + P->block_res[j]) * 4 + b.band];
        }
        if (!P->d_rate_wj) HIPCHK(ctx, hipMalloc((void **)&P->d_rate_wj, wj.size() * sizeof(double)));
        if (!P->d_rate_ws) HIPCHK(ctx, hipMalloc(&P->d_rate_ws, rate_allocate_workspace((int)n)));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));              // an allocation in flight still reads the old weights
        HIPCHK(ctx, hipMemcpy(P->d_rate_wj, wj.data(), wj.size() * sizeof(double), hipMemcpyHostToDevice));
        P->rate_wj_valid = true;
    }
    // a batch plan whose frames are allocated alone: their job ranges, and the table the _frames calls' values go through
    if (rate_frames(P) > 1 && !P->d_rate_frames) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: run the same calls once before j2k_ctx_capture_begin");
        const int F = rate_frames(P);
        std::vector<RateFrame> fr;
        if (!frame_job_ranges(P->block_tile, P->tile_count / F, F, fr)) return fail(ctx, J2K_ERR_UNSUPPORTED, "rate_per_frame: the jobs of a frame are not one contiguous range");
        if (!P->d_rate_fvals) HIPCHK(ctx, hipMalloc((void **)&P->d_rate_fvals, (size_t)F * sizeof(uint64_t)));
        const int r = upload(ctx, &P->d_rate_frames, fr);
        if (r != J2K_OK) return r;
    }
    return J2K_OK;
}
