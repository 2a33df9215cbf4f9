// j2k_plan.h -- host-side context / plan objects behind the C ABI (include/j2kgfx.h).  What a plan derives from its geometry without a device -- its
// scalars, its tables before they are uploaded -- is in plan_tables.h (no HIP there); here: the options, and what lives on the device.
// Two parts: j2k::PlanOptions, which needs nothing of HIP and is all that plan_tables.h takes of this file (J2K_PLAN_OPTIONS_ONLY), then the rest.
#ifndef J2K_PLAN_OPTIONS_H
#define J2K_PLAN_OPTIONS_H
namespace j2k {
// The options of a context that shape its plans' tables (j2k_ctx inherits them; j2k_ctx_set_option and, under J2K_TUNING=1, the environment
// set them).  The defaults are what the benchmarks measured best.
struct PlanOptions {
    int fwd_link = 1;          // forward 5-3: bands of one workgroup exchange halo rows through LDS (J2K_FWD_LINK)
    int inv_link = 1;          // same for the inverse kernels (J2K_INV_LINK)
    bool plane_wg3 = false;    // ... also level 0 of RGB triples of int32 planes (J2K_PLANE_WG3; measured equal to the general kernel on 4K frames: 43 vs 41 us)
    int plane_wg = 4;          // single-component planes (every level > 0, gray level 0) in workgroup form: waves per workgroup (J2K_PLANE_WG: 0 off, 4, 8)
    int l0_fuse = 0;           // forward levels 0 + 1 of RGBA8 frames in one launch: waves per workgroup of the fused bands (J2K_L0_FUSE: 0 off, 8, 16)
    int l0_wg = 8;             // packed RGBA8 level-0 forward, workgroup form: wavefronts per workgroup (J2K_L0_WG: 0 off, 4, 8)
    int l0_wg_invw = 4;        // ... of the inverse (J2K_L0_WG_INVW: 0 = same as the forward, 4, 8)
    bool l0_deal = true;       // J2K_L0_DEAL (0 = one contiguous chunk per XCD): the RGBA8 level-0 job table deals each XCD's short bands after its full ones (as the 9-7 tables do)
    int l0_wg97 = 8;           // lossy level-0 forward of an RGB triple, workgroup form: waves per workgroup (J2K_L0_WG97: 0 off, 6..16 even; measured 4K: 8 -> 78 us, 16 -> 88 us, general kernel 160 us)
    int plane_wg97 = 8;        // deeper 9-7 levels (single float64 planes) in workgroup form: waves per workgroup (J2K_PLANE_WG97: 0 = general kernels, 8)
    int l0_wg97_inv = 8;       // lossy level-0 inverse of an RGB triple, workgroup form: waves per workgroup (J2K_L0_WG97_INV: 0 off, 6 8 10 12)
    int l0_xcd_group = 16;     // J2K_L0_XCD_GROUP (inverse level-0 table): > 0 = bands go to the XCDs in groups of this many consecutive ones (0: one contiguous chunk of the table per XCD)
    bool l0_xcd = true;        // XCD-aware order of the workgroup jobs (J2K_L0_XCD=0: plane-major order)
    bool ht_alias = true;      // j2k_plan_encode_stream (HT): code each distinct block window once (J2K_HT_ALIAS=0: every job)
    int l0_inv_wpe = 5;        // its occupancy variant (J2K_L0_INV_WPE: 5 = all in registers, 26.4 us; 6 = odd row parked in LDS for 6 waves per SIMD, measured slower: 33.6 us)
    int l0_store = 1;          // its final-coefficient store flavour (J2K_L0_STORE: 0 plain, 1 nt, 2 sc1, 4 sc1 nt)
    int l0_scr16 = 1;          // J2K_L0_SCR16 (bit 0 forward, bit 1 inverse; 0 ... 3): packed RGBA8 forward, level 0 hands X_1 to the deep launch as int16 rows (dwt53_fwd_rgba8_wg16_kernel ->
                               // dwt53_deep_fwd16_kernel; j2k_plan::scr16_fwd says when; 0 = int32 rows, the kernels as they were).  Measured: level 0
                               // 23.0 -> 21.0 us solo, headline 82.2-83.0 -> 84.7-85.0 Gpixel/s (docs/KERNEL_NOTES.md 4ae)
    int band_prows_pix = 3;    // packed-pixel level-0 forward (J2K_BAND_PROWS_PIX)
    int band_prows_97 = 8;     // 9-7 kernels: 7 halo rows per band, so taller bands (J2K_BAND_PROWS_97)
    int band_prows_inv = 0;    // 0: same as band_prows (J2K_BAND_PROWS_INV)
    int band_prows = 5;        // pair-rows per wavefront band (tunable: J2K_BAND_PROWS)
    int use_tail = 1;          // J2K_TAIL=0: every level as its own launch (A/B)
    int mega = 0;              // J2K_MEGA: packed-RGBA8 frames: the deep levels and the level-0 bands independent of them in ONE launch per direction
                               // (dwt53_mega_*_kernel); 0 (default) = level 0 as one launch + the deep launch; 1 / 2 = job order (deep, bands, flat / deep, flat, bands).
                               // Measured (C2, one frame in flight): forward 14.3 + 23.9 us against 22.2 + 15.6, inverse 29.5 + 16.3 against 16.0 + 25.0 -- the launch's
                               // LDS size is that of its largest role (112-144 KB), so the level-0 bands run one 16-wave workgroup per CU and lose what the overlap gains
    int deep_mid_inv = 1;      // J2K_DEEP_MID_INV: the same split in the inverse launch (1 = deep + mid + flat with the compact LDS layout: two workgroups per CU, the default since round 4; 0 = deep + flat; 2 = deep + mid, flat rows inside them)
    int deep_min_planes = 12;  // J2K_DEEP_MIN_PLANES: fewer tile-components than this keep the per-level launches
    int deep_mid = 1;          // J2K_DEEP_MID=0: the deep workgroup keeps the whole top half of its plane (no mid workgroup beside it)
    int use_deep = 1;          // J2K_DEEP=0: level tail_l0 - 1 as its own launch + the LDS tail (round 2) instead of ONE launch for every level below 0 (dwt53_deep.inc)
    int xcd_map = 0;           // J2K_XCD_MAP=0: plain job order (A/B)
    int cpl0 = 0;              // J2K_CPL0: force columns-per-lane of the level-0 5-3 kernels (tuning)
    int force_novec = 0;       // J2K_FORCE_NOVEC=1: always take the scalar-access kernels (testing)
};
}  // namespace j2k
#endif

#if !defined(J2K_PLAN_OPTIONS_ONLY) && !defined(J2K_PLAN_H)
#define J2K_PLAN_H
#include <string>
#include <vector>

#include "../../include/j2kgfx.h"
#include "j2k_internal.h"
#include "plan_tables.h"
#include "graph_guard.h"

// What the MQ block coder's last launches took (j2k_plan_mq_forms / j2k_ctx_mq_forms): written where the choices are made, read by nobody else
struct j2k_mq_record {
    int enc_k = 0, enc_big2 = 0;                                   // blocks per wavefront of the MQ chains (0: the one-kernel form) / blocks above 64 x 64 through symbol lists
    int dec_split = 0, dec_lanes = 0, dec_big = 0, dec_fellback = 0;   // plane-stepped path taken, its form / launches of the big-block decoder / the path was wanted and not had
};

// (the options that shape a plan's tables: j2k::PlanOptions above)
struct j2k_ctx : j2k::PlanOptions {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string last_error;
    int fuse_compact = 0;      // j2k_plan_encode_stream: encode + compact in ONE kernel (decoupled look-back; J2K_FUSE_COMPACT=1).
                               // Measured slower than the three kernels it replaces (61.7 vs 58.6 us: the prefix chain crosses XCDs)
    int pix_fuse = 1;          // J2K_PIX_FUSE: packed pixels read / written by the level-0 kernels (1: every format; 2: RGBA8 and Gray16 only, as before round 4; 0: always the int32 staging frame)
    int ht_enc_waves = 4;      // ... with this many wavefronts per distinct window (J2K_HT_ENC_WAVES: 1 = ht_encode_kernel, 4 = ht_encode_wg_kernel)
    int ht_dec_front = 3;      // HT block decode, kernels 1 + 2 (J2K_HT_DEC_FRONT: 3 = ht_vlcprep_kernel + ht_walk_kernel, two launches; 1 = ht_front_kernel, the workgroup unstuffs the strings it walks)
    int ht_dec_lean = 1;       // HT block decode, third kernel (J2K_HT_DEC_LEAN: 1 = ht_decode_lean_kernel, the 64-wide common case written out and everything else out of line; 0 = ht_decode_kernel)
    int ht_dec_dedup = 1;      // HT block decode (J2K_HT_DEC_DEDUP, with ht_dec_front = 3 and ht_dec_lean = 1 only): 1 = a job whose bytes ht_vlcprep_kernel finds equal to its leader's
                               // (the plan's candidate table, d_ht_dec_rep) is not decoded; the leader stores its rows to both places.  Equal: in every byte a
                               // decode path can read.  The walk then takes the jobs in d_ht_walk_order (leaders first).  Measured: docs/KERNEL_NOTES.md 4aa
    bool l0_wg_inv = true;     // the inverse level 0 to RGBA8 in workgroup form too (J2K_L0_WG_INV=0: the general kernel)
    int fwd_pf = 0;            // forward 5-3 level kernels: software prefetch of the next pair-row (J2K_FWD_PF)
    int t1_split = 1;          // J2K_T1_SPLIT=0: T1 encoder as one kernel (contexts + MQ chain on lane 0) instead of two
    long t1_sym_mb = 8192;     // J2K_T1_SYM_MB: cap of the T1 symbol workspace; blocks with more bit planes than fit take the one-kernel path
    int t1_dec_general = 0;    // J2K_T1_DEC_GENERAL=1: every block on the general T1 decode kernel (A/B against t1_decode64_kernel)
    int t1_dec_lanes = 2;      // J2K_T1_DEC_LANES: 2 = the plane-stepped decoder as one launch per group of 64 blocks (t1_lanes.inc, PERSIST), 1 = its passes as launches per plane, 0 = the plane-stepped decoder's SigProp / Cleanup as round 2's step kernels (one block per wavefront) instead of t1_lanes.inc
    int t1_dec_split = -1;     // J2K_T1_DEC_SPLIT: MQ decode of frames with at least this many blocks runs plane by plane with the MagRef chains
                               // of 64 blocks per wavefront in lock step (t1.hip); 0: always the one-launch kernels; -1 (default): 512 while
                               // at least two contexts of this process code with the MQ coder (frames in flight: throughput), else 12 000 (one
                               // frame at a time: latency)
    bool capturing = false;    // between j2k_ctx_capture_begin / _end: the plan calls are recorded into a HIP graph, nothing may allocate or synchronise
    bool fault_armed_before_capture = false;
    j2k::GraphGuard guard;     // which staging slots and plans a capture used, and the generations j2k_graph_launch compares (graph_guard.h)
    bool counted_mq = false;   // this context has built an MQ-coder plan (counted in g_mq_ctxs)
    j2k_mq_record mq_forms;    // of the last j2k_decode_blocks / _coarse / _floors (the host calls have no plan)
    bool t2_parallel = true;   // J2K_T2_PARALLEL: frame decode of SOP + EPH streams parses a tile's packets side by side from their markers (verified; 0 = the tile chain only)
    int t1_lanes = 0;          // J2K_T1_LANES: blocks per wavefront of the lane-parallel MQ kernel (0: blocks / 256, at most 64, while at least two contexts code with the MQ coder, else blocks / 2048)
    // cached single-plane plans for the host (unit) calls
    std::vector<j2k_plan *> cache;
    // host-call staging buffers (device)
    void *stage[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};    // 0 / 1 staging, 2 T1 workspace, 3 fault word + results, 4 symbol lists of the big-block encoder
    bool fault_armed = false;  // a block-encode launch may have written the sticky fault word (stage[3]) since the last check
    size_t stage_bytes[5] = {0, 0, 0, 0, 0};
    // level-0 kernel timing (j2k_ctx_profile_*)
    int profile = 0;
    std::vector<hipEvent_t> ev;     // pool of event pairs
    std::vector<int> ev_tag;        // per pair: 0 = forward level 0, 1 = forward deeper levels, 2 = inverse level 0, 3 = inverse deeper levels
    size_t ev_used = 0;             // events recorded since the last read
};

namespace j2k {

struct LevelTab : LevelInfo {
    DwtPlane *d_planes = nullptr;
    DwtJob *d_jobs = nullptr;
    DwtJob *d_pjobs = nullptr; // the workgroup form's table (LevelInfo::pnjobs)
};

// the tables of one `reduce` of a Mallat plan (ReducedInfo, plan_tables.h), made at its first use
struct ReducedTab : ReducedInfo {
    bool built = false;
    LevelTab inv[2];           // the launch of level `reduce`, the final one ([0] single components, [1] MCT triples): out_off / out_stride address the reduced frame
    LLPlane *d_ll = nullptr;   // reduce == levels: no level runs (mct.hip mallat_ll_kernel)
    // the code-block jobs of the resolutions <= num_resolutions - 1 - reduce, in job order, and their share of the frame's block tables
    int *d_ids = nullptr;
    BlockJob *d_bjobs = nullptr, *d_djobs = nullptr, *d_placed = nullptr;   // windows / dense decoded blocks (the plan's offsets) / HT: the windows as destinations
    uint64_t *d_offs = nullptr; uint32_t *d_lens = nullptr; uint8_t *d_numbps = nullptr;
};

// Quality layers (j2k_plan_*_layers): the tables of one layer count L -- the stream's on the encode side, the layers read on the
// decode side (the same tables: a tile's packet sequence once per layer, the layer outermost).  Made at the first use of that L, kept in the plan.
struct LayerTab {
    bool built = false;
    int npackets = 0;                          // L x the plan's
    j2k_t2_dev_packet *d_packets = nullptr;    // J2K_T2_LAYERED set; packet (tile, l, q): layer l, cb0 = l * blocks + the plan packet's
    int *d_tile_packet0 = nullptr;             // first packet of every tile (+ the count)
    int32_t *d_ptile = nullptr;                // packet -> tile
    int *d_end_packet = nullptr;               // [tile * L + l]: the packet behind layer l of the tile (t2_layer_ends_kernel)
    j2k_t2_dev_cb *d_cbs = nullptr;            // L x blocks entries
    uint64_t *d_poffs = nullptr;               // encode: packet offsets
    void *d_ws = nullptr;                      // encode: the packet coder's workspace + its result words
    uint64_t *d_body_base = nullptr;           // decode
    uint8_t *d_kept = nullptr;                 // frame encode only, made at its first use: L x blocks cumulative cuts
};

}  // namespace j2k

// The geometry's scalars and host-side lists are j2k::PlanScalars (plan_tables.h), as build_plan_tables derived them; here: the device tables made
// of its vectors (plan_device_tables in j2k_planbuild.cpp pairs each with its vector: upload and free walk that one list), and whatever the other files make at first use
struct j2k_plan : j2k::PlanScalars {
    j2k_ctx *ctx = nullptr;
    uint64_t serial = 0;       // of ctx->guard: never reused, so a graph tells this plan from a later one at the same address (graph_guard.h)
    j2k::PlanSpec spec;
    // [cls][level]: cls 0 = single-component groups, cls 1 = MCT triples
    std::vector<j2k::LevelTab> fwd[2], inv[2];
    void *d_scrA = nullptr, *d_scrB = nullptr;   // int32 (5-3) or f64 (9-7) prefixes
    j2k::TailPlane *d_tail = nullptr;           // fused LDS tail (5-3): levels tail_l0 .. levels-1 in one launch per direction
    uint8_t *d_scr16_fmt = nullptr;             // scr16_inv: d_scr16_fmt[(element offset of a row of X_1 in scratch A) >> 3] = 1 where the row is stored as int16
    bool last_fwd_scr16 = false, last_inv_scr16 = false;   // what the plan's last forward / inverse call launched (j2k_plan_scr16 bits 2, 3)
    j2k::TailPlane *d_deep_planes = nullptr;    // dims at level deep_l0
    j2k::DwtJob *d_deep_jobs = nullptr;         // deep workgroups first, then the flat ones
    j2k::DwtJob *d_deep_jobs_inv = nullptr;     // the inverse launch's table (deep / mid jobs own other level-l0 rows than in the forward one)
    // merged launches for packed RGBA8 frames (dwt53_mega_*_kernel) and the level-0 TOP band tables that go with them
    j2k::DwtJob *d_mega_fwd_jobs = nullptr, *d_mega_inv_jobs = nullptr, *d_fwd_top_jobs = nullptr, *d_inv_top_jobs = nullptr;
    // closed-loop frame codec (j2k_plan_encode_tile_parts / j2k_plan_decode_tile_parts): tables and workspaces, made at first use
    j2k_t2_dev_packet *d_t2_packets = nullptr;   // one packet per (tile, component, resolution) with blocks, J2K_T2_* flags set
    int *d_tile_packet0 = nullptr;               // first packet of every tile of the shard (+ the packet count)
    int t2_npackets = 0;
    j2k_t2_dev_cb *d_t2_cbs = nullptr;           // code-block table of the packet coder / decoder (one entry per job)
    uint64_t *d_t2_poffs = nullptr;              // encode: where each packet starts among the packets (+ their total)
    int t2_body_slices = 8;
    int32_t *d_t2_ptile = nullptr;               // encode: packet -> tile (its place in the tile-parts is 14 (tile + 1) bytes further)
    void *d_t2_ws = nullptr;                     // encode: the packet coder's workspace + its 3-word result
    void *d_t2_chains = nullptr;                 // decode: one chain per tile
    uint64_t *d_t2_body_base = nullptr;          // decode: where each packet's bodies start
    void *d_t2_par = nullptr;                    // decode: one chain per PACKET, the marker lists and guesses (t2_par_workspace)
    int *d_frame_status = nullptr;               // sticky status word of the asynchronous frame calls (j2k_plan_frame_status)
    int32_t *d_cl_decoded = nullptr, *d_cl_coeff = nullptr;   // j2k_plan_*_frame_pixels: decoded blocks, coefficient planes
    int32_t *d_cl_coeff_dec = nullptr;           // HT plans: the frame DECODER's coefficient planes (zeroed once, only the coded rows ever written)
    uint8_t *d_cl_numbps = nullptr; uint64_t *d_cl_offs = nullptr; uint32_t *d_cl_lens = nullptr;
    void *d_host_io = nullptr, *d_host_pix = nullptr;          // j2k_encode_pixels_host / j2k_decode_pixels_host: tile-parts / pixels on the device
    size_t host_io_bytes = 0, host_pix_bytes = 0;
    int *d_tile_job0 = nullptr;             // first job of each tile of the shard (+ the job count): j2k_plan_assemble_tiles_device
    j2k::BlockJob *d_bjobs = nullptr;       // out_off = slot byte offset (encode)
    j2k::BlockJob *d_djobs = nullptr;       // out_off = decoded element offset (decode)
    j2k::BlockJob *d_djobs_placed = nullptr; // closed-loop HT plans: out_off = the block's window in the coefficient planes, stride = the plane's
    // device workspaces owned by the plan for j2k_encode_frame
    void *d_frame = nullptr, *d_coeff = nullptr, *d_slots = nullptr, *d_stream = nullptr;
    void *d_lens = nullptr, *d_numbps = nullptr, *d_offs = nullptr;
    // fused encode + compact (j2k_plan_encode_stream): look-back status words, tagged with the launch epoch
    j2k::DwtJob *d_fwd_pix_jobs = nullptr;  // level-0 forward job table of the packed-pixel path (shorter bands)
    j2k::HtUJob *d_ht_ujobs = nullptr; int *d_ht_alias_next = nullptr;   // HT: one entry per distinct window / the job ids sharing each window
    j2k::BlockJob *d_bjobs_alias = nullptr;                  // d_bjobs with every job's slot = the slot of its window's coded job
    // HT decode, byte-identical blocks (option ht_dec_dedup): CANDIDATES only -- the prep kernel compares the bytes.  d_ht_dec_rep[j] = the leader of job j (the
    // lowest job with the same window that it may follow; j itself otherwise), d_ht_dec_fol[8 j] = how many jobs follow leader j (at most J2K_HT_DEC_MAX_FOLLOWERS),
    // d_ht_dec_fol[8 j + 1 ..] = their ids.  Both null when no job has a follower (closed-loop plans: the windows partition the plane).
    int32_t *d_ht_dec_rep = nullptr, *d_ht_dec_fol = nullptr;
    // The walk's static order under the same option: slot s of the bit-string scratch (and lane s % 64 of walk workgroup s / 64) belongs to job
    // ht_walk_order[s] -- the ht_walk_nlead jobs that are their own leader first, in ascending job order, the static followers behind them, ascending;
    // d_ht_walk_pos is the inverse (job -> slot).  Uploaded with d_ht_dec_rep; the identity, and null, when no job has a follower.
    int32_t *d_ht_walk_order = nullptr, *d_ht_walk_pos = nullptr;
    j2k::DwtJob *d_fwd97_wg_jobs = nullptr; // 9-7: one job per workgroup = (plane, component, band) of dwt97_fwd_rgb_wg_kernel
    j2k::DwtJob *d_inv97_wg_jobs = nullptr; // 9-7 inverse: one job per workgroup = (plane, band) of dwt97_inv_rgb_wg_kernel
    j2k::DwtJob *d_fwd_wg2_jobs = nullptr, *d_fwd_wg_rest_jobs = nullptr;   // fused levels 0+1: top-half bands / the remaining bands
    j2k::DwtJob *d_fwd_wg_jobs = nullptr;   // the same as one job per WORKGROUP (dwt53_fwd_rgba8_wg_kernel), when every plane qualifies
    j2k::DwtJob *d_inv_wg_jobs = nullptr;   // the inverse kernel's table (its own waves per workgroup)
    uint32_t *d_maglens = nullptr;          // j2k_plan_encode_stream: end of each block's MagSgn bytes (the MEL hole starts there)
    uint32_t *d_mels = nullptr;      // per job: bytes of MEL zero run of an HT block (max(64, 2wh) / 4), built with d_maglens
    const void *last_stream = nullptr, *last_lens = nullptr;   // outputs of the last j2k_plan_encode_stream: what d_maglens / d_toffs describe
    bool want_toffs = false, toffs_valid = false;   // pack_stream has been used on this plan / d_toffs belongs to the last encode_stream
    uint64_t *d_toffs = nullptr;     // n + 1: exclusive scan of the transport lengths of the last j2k_plan_encode_stream (pack_stream)
    uint64_t *d_status = nullptr;
    uint32_t epoch = 0;
    bool all_blocks_fast = false;           // every job on the parallel HT path
    uint64_t *d_bigsym_off = nullptr;       // MQ plans with blocks above 64 x 64: where each job's symbol list starts (bytes; n + 1 entries), built at the first encode
    size_t bigsym_total = 0;
    bool dec_coded_rows_only = false;       // j2k_plan_set_decode_coded_rows_only: HT decode leaves the rows the reference's decoder never writes alone
    std::vector<j2k::ReducedTab> reduced;   // Mallat plans: [reduce], 1 ... levels
    // rate control (j2k_plan_rate_allocate): one weight per (component, resolution, band), index (c * num_res_jobs + r) * 4 + band; the default is the
    // band's synthesis energy gain on a Mallat plan and 1 elsewhere (plan_default_rate_weights); d_rate_wj = the weight of every job, uploaded
    // at the first allocation after the table changed
    std::vector<double> rate_weights;
    double *d_rate_wj = nullptr;
    bool rate_wj_valid = false;
    void *d_rate_ws = nullptr;              // the allocation kernel's hulls
    // j2k_plan_set_rate_per_frame: every rate call allocates each frame of a batch alone (tests/frame_rate_cases.py).  d_rate_frames: the job
    // range of every frame (plan_tables.h: frame_job_ranges), uploaded at the first rate call with the setting on; d_rate_fvals: one 64-bit
    // value per frame, the budgets or targets of the _frames calls (written on the stream by launch_rate_frame_values)
    bool rate_per_frame = false;
    j2k::RateFrame *d_rate_frames = nullptr;
    uint64_t *d_rate_fvals = nullptr;
    void *d_cl_prate = nullptr;             // the *_passes frame calls: the 96-entry rate and distortion tables and the SigProp masks (cl_rate_workspace)
    void *d_cl_rate = nullptr;              // the *_rate frame calls: rate and distortion tables, kept planes, chosen bytes, floors (cl_rate_workspace)
    std::vector<j2k::LayerTab> layer_tabs;  // quality layers: [L], 1 ... J2K_MAX_LAYERS
    void *d_cl_dense = nullptr;             // j2k_plan_decode_frame_pixels_layers: the gathered codewords (at least the stream's length) ...
    size_t cl_dense_bytes = 0;
    uint8_t *d_cl_lfloors = nullptr;        // ... and the blocks' floors (whole frame | the subset of a reduced decode)
    // region decode (j2k_area.cpp), made at the first area call: the jobs' windows and every plane's tile rectangle for area_blocks_kernel, and the
    // int32 staging frame [C][H][W] the whole-frame inverse writes before the window is packed
    j2k_block *d_area_blocks = nullptr;
    j2k::AreaPlane *d_area_planes = nullptr;
    int32_t *d_area_frame = nullptr;
    bool raw_magref = false;                // j2k_plan_set_raw_magref: MQ block bodies are H | MQ | RAW, the MagRef decisions bypass the MQ coder
    j2k_mq_record mq_forms;                 // of the plan's last block encode / block decode (j2k_plan_mq_forms)
    bool dequantize = false;                // j2k_plan_set_dequantize: the 9-7 inverse kernels multiply every int32 coefficient by 1.0 / Quality at their load (dwt.go:514-520)
};
#endif  // J2K_PLAN_H
