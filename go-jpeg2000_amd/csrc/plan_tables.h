// plan_tables.h -- a frame geometry compiled into job tables, on the host and without HIP: what a plan is made of before anything is uploaded.
// build_plan (j2k_planbuild.cpp) calls build_plan_tables, uploads every vector of the PlanTables it gets and keeps its scalars;
// tests/plan_tables_main.cpp calls the same function on a CPU, under sanitizers, and pins every table to a recording.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/j2kgfx.h"
#include "j2k_tables.h"
#ifndef J2K_PLAN_H                 // (not from inside j2k_plan.h itself:) j2k::PlanOptions, the one part of that header that needs no HIP
#define J2K_PLAN_OPTIONS_ONLY
#include "j2k_plan.h"
#undef J2K_PLAN_OPTIONS_ONLY
#endif

namespace j2k {

enum Wavelet { W53 = 0, W97 = 1 };
enum QuantMode {               // how the 9-7 path turns f64 coefficients into int32
    Q_NONE = 0,                // keep f64 (dwt.Forward97... unit calls)
    Q_ENCODER = 1,             // int32(v/step +- 0.5), step = 1/quality (encoder.go:265-276)
    Q_TCD = 2                  // int32(v +- 0.5) (tcd.go:520-532)
};
static_assert(sizeof(Wavelet) == 4 && sizeof(QuantMode) == 4 && W97 == 1 && Q_TCD == 2, "PlanSpec keeps these as int");

// Internal, richer form of j2k_params.
struct PlanSpec {
    int W = 0, H = 0, C = 1;
    int tile_w = 0, tile_h = 0;
    int levels = 1;            // DWT levels actually run
    int wavelet = W53;
    int precision = 8;         // component precision of the plan (pixel pack / unpack)
    int dc_shift = 0;          // value subtracted on the way in (encoder.go:218-220)
    int dc_shift_inv = 0;      // value added on the way out: 0 for signed components (decoder.go:344-348), else dc_shift
    int mct = 0;               // fused RCT (W53) / ICT (W97) on comps 0-2 when C>=3
    int quant = Q_NONE;
    int quality = 100;
    int num_res_jobs = 6;      // resolutions for the encodeTile job enumeration
    int cb_w = 64, cb_h = 64;
    int coder = J2K_CODER_MQ;
    int frame_h = 0;           // rows of one frame of a batch (j2k_params.frame_rows; = H for a single frame)
    int tile_first = 0, tile_count = 0;
    bool frame_is_f64 = false; // unit 9-7 calls: source/destination "frame" is f64
    bool closed_loop = false;  // j2k_params.closed_loop: code-block windows = the Mallat rectangles of the plane (they partition it)
    bool mallat = false;       // j2k_params.closed_loop == J2K_CLOSED_LOOP_MALLAT: level l runs on the rectangle [0, w_l) x [0, h_l) of the plane, so those windows are its sub-bands
    bool operator==(const PlanSpec &o) const;
};

struct Group {                 // one launch unit: a single component or an MCT triple of one tile
    int tile;                  // shard-local tile index
    int comp0, nc;
    int x0, y0, w, h;
    int64_t coef_off[3];       // element offsets into the coefficient buffer
    int64_t scrA_off[3], scrB_off[3];
};
J2K_TABLE_LAYOUT(PlanSpec, 84, mallat, 82);
J2K_TABLE_LAYOUT(Group, 104, scrB_off, 80);

// what the HT decode kernels can take on their parallel path (ht.hip: ht_fast_max_samples(), ht_walk_max_pairs())
struct PlanLimits { int ht_fast_max_samples = 0, ht_walk_max_pairs = 0; };

// One level of one class of groups: what the launch needs to know about its tables
struct LevelInfo {
    int njobs = 0, nplanes = 0;
    int cpl = 2, vec = 0, ncomp = 1;
    int64_t alg_bytes = 0;
    // single-component planes in workgroup form (dwt53_plane_wg.inc): one entry per (plane, 512-column strip, band of
    // pwaves - 1 pair-rows); empty when a plane of the level breaks the geometry contract
    int pnjobs = 0, pwaves = 0, pmulti = 0;
    bool p_pix_only = false;   // the table serves packed-pixel sources only (level 0 of RGB triples: RGBA64); int32 planes keep the general kernels
    bool mallat = false;       // a level of a Mallat plan: the MAL instantiation of the general kernels (LevelLaunch::mallat)
};
struct LevelTables : LevelInfo { std::vector<DwtPlane> planes; std::vector<DwtJob> jobs, pjobs; };

// Everything a plan derives from its geometry that is not a device table: the plan keeps these as they are (j2k_plan inherits them)
struct PlanScalars {
    int tiles_x = 1, tiles_y = 1, tile_first = 0, tile_count = 1;
    std::vector<Group> groups;
    std::vector<int64_t> plane_desc;        // 7 x int64 per tile-component
    int64_t coeff_elems = 0, scrA_elems = 0, scrB_elems = 0;
    // fused LDS tail (5-3): levels tail_l0 .. levels-1 in one launch per direction; -1 = not used
    int tail_l0 = -1;
    int ntail = 0;
    size_t tail_lds_fwd = 0, tail_lds_inv = 0;
    // every level below level 0 in one launch per direction (dwt53_deep.inc): levels deep_l0 .. levels-1; -1 = not used
    int deep_l0 = -1;
    bool scr16_inv = false;                     // inverse_rgba8 of this plan may: rows of X_1 that fit int16 are stored so, d_scr16_fmt[(element offset of the row) >> 3] = 1 says which
    bool scr16_fwd = false;                     // forward_rgba8 of this plan may hand X_1 over as int16 rows (option l0_scr16; the conditions: plan_tables.cpp)
    int ndeep_jobs = 0, ndeep_jobs_inv = 0;
    size_t deep_lds = 0, deep_lds_fwd = 0;      // dynamic LDS of the inverse / forward launch
    int mega_fwd_njobs = 0, mega_inv_njobs = 0, fwd_top_njobs = 0, inv_top_njobs = 0;
    int64_t fwd_top_bytes = 0, inv_top_bytes = 0;        // algorithmic bytes of the top-band launches (16 B per pixel)
    // code-block jobs
    std::vector<j2k_block> blocks;          // plane = shard-local tile-component index
    std::vector<int32_t> block_tile;        // tile of each job
    std::vector<int32_t> block_res;         // resolution of each job (a packet = the jobs of one tile-component and resolution)
    int max_block_h = 0;
    uint64_t max_tile_bytes = 0;            // slot bytes of the largest tile (an upper bound of its stream bytes)
    std::vector<uint64_t> slot_off;         // byte offset of each job's worst-case slot
    std::vector<uint64_t> dec_off;          // element offset of each job's decoded block
    int64_t bytes_cap = 0, decoded_elems = 0, block_samples = 0;
    int64_t dwt_bytes = 0, dwt_level0_bytes = 0;
    int fwd_pix_njobs = 0;
    int ht_nunique = 0;
    std::vector<int32_t> ht_dec_rep;        // the host's copy of d_ht_dec_rep (every HT plan; j2k_plan_get_ht_decode_leaders)
    std::vector<int32_t> ht_walk_order;     // the host's copy (every HT plan; j2k_plan_get_ht_decode_walk_order)
    int ht_walk_nlead = 0;
    int fwd97_wg_njobs = 0, fwd97_wg_waves = 0;
    int inv97_wg_njobs = 0, inv97_wg_waves = 0;
    int fwd_wg2_njobs = 0, fwd_wg2_waves = 0, fwd_wg_rest_njobs = 0;
    int fwd_wg_njobs = 0, fwd_wg_waves = 0;
    int inv_wg_njobs = 0, inv_wg_waves = 0;
};

// ... and the device tables, as they will be uploaded: a plan has the form a table serves exactly when the table is not empty (an empty vector
// is a null device pointer, which is what the launch code tests).  Each is described at its device pointer in j2k_plan.h.
struct PlanTables : PlanScalars {
    std::vector<LevelTables> fwd[2], inv[2];        // [cls][level]: cls 0 = single-component groups, cls 1 = MCT triples
    std::vector<TailPlane> tail, deep_planes;
    std::vector<DwtJob> deep_jobs, deep_jobs_inv;
    std::vector<DwtJob> mega_fwd_jobs, mega_inv_jobs, fwd_top_jobs, inv_top_jobs;
    std::vector<DwtJob> fwd_pix_jobs, fwd_wg_jobs, inv_wg_jobs, fwd_wg2_jobs, fwd_wg_rest_jobs, fwd97_wg_jobs, inv97_wg_jobs;
    std::vector<int> tile_job0;
    std::vector<BlockJob> bjobs, djobs, djobs_placed, bjobs_alias;
    std::vector<HtUJob> ht_ujobs;
    std::vector<int> ht_alias_next;
    std::vector<int32_t> ht_dec_fol, ht_walk_pos;
    bool ht_dec_any = false;                        // some job has a follower: ht_dec_rep and ht_walk_order are device tables too (else the identity, not uploaded)
};

// S -> T.  J2K_OK, or J2K_ERR_INVALID_ARG with *why = "bad geometry" / "plane too large"
int build_plan_tables(const PlanOptions &o, const PlanLimits &lim, const PlanSpec &S, PlanTables &T, const char **why);

// The job range of every frame of a batch for the rate allocation (j2k_plan_set_rate_per_frame; tests/frame_rate_cases.py: frame_ranges): frame f
// owns the blocks whose tile is in [f * tiles_per_frame, (f + 1) * tiles_per_frame).  block_tile lists the tile of every job and must not fall
// (block_jobs emits tile by tile), so the ranges are contiguous and in order; false, with `out` empty, if it does, if a tile is outside
// [0, nframes * tiles_per_frame) or the counts are not positive.  A frame without blocks has count 0 and starts where the next one does.
bool frame_job_ranges(const std::vector<int32_t> &block_tile, int tiles_per_frame, int nframes, std::vector<RateFrame> &out);

// A Mallat plan decoded `reduce` resolutions down (j2k_plan_*_reduced): LL_reduce is the frame, W_r x H_r = ceil(W / 2^reduce) x ceil(H / 2^reduce),
// tile (x0, y0) at (x0 >> reduce, y0 >> reduce)
struct ReducedInfo {
    int Wr = 0, Hr = 0;
    int nll = 0, ll_samples = 0;
    int njobs = 0, max_block_h = 0;
};
struct ReducedTables : ReducedInfo {
    LevelTables inv[2];
    std::vector<LLPlane> ll;
    std::vector<int> ids;
    std::vector<BlockJob> bjobs, djobs, placed;
};
// J2K_OK, or the refusal of a `reduce` the plan does not allow (status, *why): J2K_ERR_UNSUPPORTED on a plan that is not Mallat,
// J2K_ERR_INVALID_ARG for a `reduce` the geometry does not allow.  build_reduced_tables makes the same check; reduce == 0 builds nothing.
int check_reduce(const PlanSpec &S, int reduce, const char **why);
int build_reduced_tables(const PlanOptions &o, const PlanSpec &S, const PlanScalars &P, int reduce, ReducedTables &R, const char **why);

}  // namespace j2k
