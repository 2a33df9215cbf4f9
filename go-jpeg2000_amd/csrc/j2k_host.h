// j2k_host.h -- what the host-side files of the C ABI share (j2k_ctx.cpp, j2k_planbuild.cpp, j2k_stages.cpp, j2k_frame.cpp, j2k_rate.cpp,
// j2k_layers.cpp, j2k_area.cpp, j2k_hostcalls.cpp, j2k_pipe.cpp; round 4 had all of it in one 2 200-line j2k_abi.cpp): the kernels' launch wrappers, the
// status helpers, the context's staging slots, the plan builder, and the requests, the one encoder / decoder and the two host drivers of the
// closed-loop frame codec.  Host-side orchestration only: geometry -> device job tables, launches on the
// context's HIP stream, host <-> device staging.  All arithmetic lives in the .hip kernels; there is no CPU fallback.
// A plan is made in three steps (j2k_planbuild.cpp: build_plan): build_plan_tables (plan_tables.h / plan_tables.cpp: plain integer code with no HIP
// in it, run on a CPU under sanitizers by tests/plan_tables_main.cpp) turns the geometry and the context's PlanOptions into every job table and
// scalar; one list of (device pointer, host vector) pairs uploads the tables -- and frees them in j2k_plan_destroy; the scratch buffers are allocated.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <tuple>

#include "j2k_plan.h"

namespace j2k {
#ifdef J2K_DEV
int g_dev_skip = 0, g_dev_dup = 0;
#endif
hipError_t launch_add_const(hipStream_t s, int32_t *d, size_t n, int delta);
hipError_t launch_rct(hipStream_t s, int32_t *a, int32_t *b, int32_t *c, size_t n, int inverse);
hipError_t launch_ict(hipStream_t s, double *a, double *b, double *c, size_t n, int inverse);
hipError_t launch_dwt97_fwd(hipStream_t s, const LevelLaunch &L, const void *src, int src_is_f64, int32_t *out_i32,
                            double *out_f64, double *nxt, int dc_shift, int quant, double step, int mct);
hipError_t launch_dwt97_inv(hipStream_t s, const LevelLaunch &L, const void *coef, int coef_is_f64, const double *prev,
                            void *dst, int dc_shift, int final_level, int dst_mode, int mct, double step);
hipError_t launch_quantize97(hipStream_t s, const double *src, size_t n, double step, int32_t *dst);
hipError_t launch_dequantize97(hipStream_t s, const int32_t *src, size_t n, double step, double *dst);
hipError_t launch_ht_encode(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, uint8_t *slots,
                            uint32_t *lens, uint8_t *numbps, int *fault, uint32_t *maglens = nullptr, const HtUJob *utab = nullptr, int nunique = 0,
                            const int *alias_ids = nullptr, int waves = 1);
hipError_t launch_ht_decode(hipStream_t s, const BlockJob *jobs, int njobs, const uint8_t *stream, const uint64_t *offs,
                            const uint32_t *lens, int32_t *decoded, uint32_t *scratch, int coded_rows_only = 0, const BlockJob *placed_jobs = nullptr, int lean = 1, int front = 3,
                            const int32_t *dedup_rep = nullptr, const int32_t *dedup_fol = nullptr, const int32_t *walk_order = nullptr,
                            const int32_t *walk_pos = nullptr, int walk_nlead = 0);
int ht_walk_max_pairs();
size_t ht_decode_scratch_words(int njobs);
hipError_t launch_ht_encode_stream(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, uint8_t *stream,
                                   uint64_t *offs, uint32_t *lens, uint8_t *numbps, uint64_t *status, uint32_t epoch, int *fault);
int ht_fast_max_samples();
hipError_t launch_t1_encode(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, uint8_t *slots,
                            uint32_t *lens, uint8_t *numbps, uint8_t *work, size_t work_per_job, int *fault, int max_dim,
                            uint8_t *sym, size_t sym_stride, uint32_t *nsyms, int lanes, uint8_t *bigsym = nullptr, const uint64_t *bigsym_off = nullptr,
                            uint32_t *bignsyms = nullptr, uint32_t *rate = nullptr,    // rate: 32 words per job, the rate tables (blocks <= 64 x 64 only)
                            uint32_t *rawst = nullptr,    // rawst: the raw-MagRef style -- t1_raw_stage_bytes() per job of staging (blocks <= 64 x 64, no rate tables)
                            int *forms = nullptr,         // forms (host, two ints): [0] = blocks per wavefront of the MQ chains (0: the one-kernel form), [1] = 1: blocks above 64 x 64 went through symbol lists
                            uint64_t *spmask = nullptr);  // spmask (with rate): the pass tables -- rate has 96 words per job, spmask 64 row masks per job (blocks <= 64 x 64 only)
size_t t1_raw_stage_bytes();
// rate control (rate.hip): plane distortions of every block; the allocation of a byte budget over the blocks' rate / distortion tables
hipError_t launch_rate_distortion(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, uint64_t *dist);
// pass cuts (tests/pass_cases.py): tables of 96 entries per block; spmask: 64 row masks per block (t1.hip's PASSES instantiations)
hipError_t launch_rate_distortion_passes(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, const uint64_t *spmask,
                                         uint64_t *dist);
hipError_t launch_rate_allocate_passes(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                       uint64_t budget, void *ws, uint8_t *kept, uint64_t *chosen, int nframes = 1, const RateFrame *frames = nullptr,
                                       const uint64_t *frame_budgets = nullptr);
hipError_t launch_rate_allocate_quality_passes(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                               double target, void *ws, uint8_t *kept, uint64_t *chosen, double *achieved, int nframes = 1,
                                               const RateFrame *frames = nullptr, const double *frame_targets = nullptr);
// region of interest (area.hip, rate.hip): every block's footprint of a rectangle; the distortions with that footprint weighted `gain` times
hipError_t launch_roi_windows(hipStream_t s, const j2k_block *blocks, int n, const AreaPlane *planes, int x0, int y0, int x1, int y1, int margin, int32_t *win);
hipError_t launch_rate_distortion_roi(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, const j2k_block *blocks,
                                      const AreaPlane *planes, int x0, int y0, int x1, int y1, int margin, uint32_t gain, uint64_t *dist);
size_t rate_allocate_workspace(int njobs);
// A batch plan with j2k_plan_set_rate_per_frame: `frames` (device) = the job range of each of its nframes frames, one workgroup per frame, kept
// [layers][njobs], chosen and achieved [layers][nframes]; frame_budgets / frame_targets (device, or null; one layer): frame f's own value in the
// place of the scalar.  frames == NULL: one frame of all njobs jobs, as ever.
hipError_t launch_rate_allocate(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                uint64_t budget, void *ws, uint8_t *kept, uint64_t *chosen, int nframes = 1, const RateFrame *frames = nullptr,
                                const uint64_t *frame_budgets = nullptr);
hipError_t launch_rate_allocate_layers(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                       const uint64_t *budgets, int nlayers, void *ws, uint8_t *kept, uint64_t *chosen, int nframes = 1,
                                       const RateFrame *frames = nullptr);
// nframes 64-bit values of the host (budgets, or the bits of float64 targets) into a device table, by value: a captured call replays them
hipError_t launch_rate_frame_values(hipStream_t s, const uint64_t *values, int nframes, uint64_t *table);
// the dual (rate.hip): per layer the fewest bytes whose weighted distortion stays within targets[l]; achieved[l] = that distortion
hipError_t launch_rate_allocate_quality(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                        const double *targets, int nlayers, void *ws, uint8_t *kept, uint64_t *chosen, double *achieved, int nframes = 1,
                                        const RateFrame *frames = nullptr, const double *frame_targets = nullptr);
// per-channel sums of squared sample differences of two frames in one Pix layout (pixels.hip)
size_t pixels_sse_workspace();
hipError_t launch_pixels_sse(hipStream_t s, const uint8_t *a, size_t stride_a, const uint8_t *b, size_t stride_b, size_t rowbytes, int h, bool wide, int channels,
                             uint64_t *partial, uint64_t *sums);
// quality layers (t2dev.hip, t2dec.hip)
hipError_t launch_t2_fill_layer_cbs(hipStream_t s, long n, int nlayers, const uint64_t *offs, const BlockJob *slot_jobs, const uint32_t *lens, const uint8_t *numbps,
                                    int mb, const uint8_t *kept, const uint32_t *rate, j2k_t2_dev_cb *cbs, uint64_t *reset);
hipError_t launch_t2_layer_ends(hipStream_t s, int count, int nlayers, const int *end_packet, const uint64_t *poffs, uint64_t *layer_offs);
hipError_t launch_t2_decode_tiles_layers(hipStream_t s, void *chains, int ntiles, const j2k_t2_dev_packet *packets, long npackets, j2k_t2_dev_cb *cbs, long n,
                                         int nlayers, const uint8_t *data, uint64_t len, int sop, int eph, uint64_t *body_base, int *frame_status, int mb,
                                         uint8_t *dense, uint64_t dense_cap, uint64_t *offs, uint32_t *lens, uint8_t *numbps, uint8_t *floors);
size_t t1_sym_stride(int planes);
hipError_t launch_t1_decode(hipStream_t s, const BlockJob *jobs, int njobs, const uint8_t *stream, const uint64_t *offs,
                            const uint32_t *lens, const uint8_t *numbps, int32_t *decoded, uint8_t *work,
                            size_t work_per_job, int max_dim, int general_only, uint8_t *split_ws, int sig_lanes, int throughput = 0, int skip_planes = 0,
                            const uint8_t *floors = nullptr,    // floors (device, one byte per job): job j stops at max(skip_planes, floors[j])
                            int raw_magref = 0,                 // the bodies are H | MQ | RAW (blocks <= 64 x 64, no floors)
                            int *big_launches = nullptr,        // (host) launches of t1_decode_big_kernel: 0, 1 or 2
                            const uint8_t *pfloors = nullptr);  // pfloors (device, one byte per job; blocks <= 64 x 64): job j stops max(3 skip_planes, pfloors[j]) coding passes short
size_t t1_dec_split_bytes(size_t njobs, bool raw_magref = false);    // raw_magref: with the un-stuffed RAW strings of the style's blocks
hipError_t launch_mq_encode(hipStream_t s, const uint8_t *ctxs, const uint8_t *decs, size_t n, uint8_t *out, size_t cap, uint32_t *out_len, int *fault);
hipError_t launch_mq_decode(hipStream_t s, const uint8_t *data, size_t len, const uint8_t *ctxs, size_t n, uint8_t *decs, int *fault);
hipError_t launch_raw_encode(hipStream_t s, const uint8_t *bits, size_t n, uint8_t *out, size_t cap, uint32_t *out_len, int *fault);
hipError_t launch_raw_decode(hipStream_t s, const uint8_t *data, size_t len, size_t n, uint8_t *bits);
size_t t1_work_bytes(int w, int h);
size_t t1_flag_bytes(int w, int h);
hipError_t launch_compact(hipStream_t s, const BlockJob *jobs, int njobs, const uint8_t *slots, const uint32_t *lens,
                          uint64_t *offs, uint8_t *stream, const uint32_t *maglens, const uint32_t *mels = nullptr, uint64_t *toffs = nullptr);
hipError_t launch_mel_table(hipStream_t s, const BlockJob *jobs, int njobs, uint32_t *mels);
hipError_t launch_assemble_tiles(hipStream_t s, const uint8_t *stream, const uint64_t *offs, const int *job0, int ntiles, int tile_first,
                                 uint64_t max_tile_bytes, uint8_t *out, uint64_t *out_len);
// t2dec.hip
size_t t2_chain_bytes();
hipError_t launch_t2_tile_chains(hipStream_t s, const uint8_t *cs, uint64_t len, const uint64_t *tile_offs, int ntiles, int tile_first,
                                 const int *tile_packet0, void *chains);
hipError_t launch_t2_decode_packets(hipStream_t s, void *chains, int nchains, const j2k_t2_dev_packet *packets, long npackets, j2k_t2_dev_cb *cbs, uint64_t ncbs,
                                    const uint8_t *data, int sop, int eph, int clean, uint64_t *body_base, int *frame_status);
void t2_make_chain(void *dst, uint64_t len, long npackets, const j2k_t2_dec_state &st);
void t2_read_chain(const void *src, j2k_t2_dec_state &st, int &status, long &done);
size_t t2_par_workspace(long npackets, int ntiles);
hipError_t launch_t2_decode_tiles(hipStream_t s, void *chains, int ntiles, const int *tile_packet0, const j2k_t2_dev_packet *packets, long npackets, j2k_t2_dev_cb *cbs,
                                  uint64_t ncbs, const uint8_t *data, uint64_t len, int sop, int eph, uint64_t *body_base, int *frame_status, void *ws,
                                  int ht, int mb, uint64_t *offs, uint32_t *lens, uint8_t *numbps, uint8_t *floors = nullptr,    // floors: t2_block_out's per-block floors (the _floors calls)
                                  uint8_t *pfloors = nullptr);                                                                  // pfloors: the same in coding passes (the _pfloors calls)
hipError_t launch_t2_blocks(hipStream_t s, long n, const j2k_t2_dev_cb *cbs, int ht, int mb, uint64_t total, uint64_t *offs, uint32_t *lens, uint8_t *numbps, int *status, uint8_t *floors = nullptr);
hipError_t launch_place_blocks(hipStream_t s, const BlockJob *src_jobs, const BlockJob *dec_jobs, int njobs, int max_h, const int32_t *decoded, int32_t *coeff, int ystep = 1);
hipError_t launch_select_blocks(hipStream_t s, const int *ids, int m, const uint64_t *offs, const uint32_t *lens, const uint8_t *numbps, uint64_t *offs_r,
                                uint32_t *lens_r, uint8_t *numbps_r);
hipError_t launch_mallat_ll(hipStream_t s, const LLPlane *planes, int nplanes, int max_samples, const int32_t *coef, int32_t *frame, int lossy, double step,
                            int dc_shift);
hipError_t launch_scan(hipStream_t s, const uint32_t *lens, int njobs, uint64_t *offs, const uint32_t *mels, uint64_t *toffs);
size_t pack_header_bytes(size_t n);
hipError_t launch_pack(hipStream_t s, const BlockJob *jobs, int njobs, const uint8_t *stream, const uint64_t *offs, const uint64_t *toffs,
                       const uint32_t *lens, const uint8_t *numbps, const uint32_t *maglens, uint8_t *pack);
hipError_t launch_unpack(hipStream_t s, const BlockJob *jobs, int njobs, int count, const uint8_t *const *packs, const size_t *pack_bytes,
                         uint8_t *const *streams, size_t stream_cap, uint64_t *const *offs, uint32_t *const *lens, uint8_t *const *numbps, int *fault);
}  // namespace j2k

// ---- status / errors (j2k_ctx.cpp) ----
int fail(j2k_ctx *ctx, int status, const char *msg);
int fail_hip(j2k_ctx *ctx, hipError_t e, const char *where);
#define HIPCHK(ctx, call)                                      \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return fail_hip(ctx, e_, #call); \
    } while (0)
// contexts of this process that have built an MQ-coder plan: two or more = frames in flight (throughput settings of the MQ kernels)
extern std::atomic<int> g_mq_ctxs;
bool mq_throughput_mode();
int check_fault(j2k_ctx *ctx);
bool profile_pair(j2k_ctx *ctx, int tag, hipEvent_t &e0, hipEvent_t &e1);
int stage_reserve(j2k_ctx *ctx, int slot, size_t bytes);
// The first statement of EVERY entry point of the C ABI whose first parameter is `j2k_plan *P` (tests/test_graph_guard.py reads the sources for
// it): while the plan's context captures, the graph records this plan's tables and workspaces, so the plan is noted for the graph's snapshot
// (graph_guard.h).  At the entry points and not further in, so that no call family can reach a launch around it; the entry points that take a
// `const j2k_plan *` are queries and launch nothing.  Costs one test of a bool outside a capture.
static inline void graph_note_plan(const j2k_plan *P) {
    if (P && P->ctx && P->ctx->capturing) P->ctx->guard.plan_used(P->serial);
}

// ---- plans (j2k_planbuild.cpp; the tables themselves: plan_tables.h) ----
static inline int64_t align4(int64_t v) { return (v + 3) & ~int64_t(3); }
template <typename T>
static int upload(j2k_ctx *ctx, T **dptr, const std::vector<T> &v) {
    *dptr = nullptr;
    if (v.empty()) return J2K_OK;
    HIPCHK(ctx, hipMalloc((void **)dptr, v.size() * sizeof(T)));
    HIPCHK(ctx, hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return J2K_OK;
}
int build_plan(j2k_ctx *ctx, const j2k::PlanSpec &S, j2k_plan **out);
int cached_plan(j2k_ctx *ctx, const j2k::PlanSpec &S, j2k_plan **out);
void plan_t2_packets(const j2k_plan *P, int layer, std::vector<j2k_t2_dev_packet> &out, std::vector<int> *tile_packet0);
// the tables of a Mallat plan decoded `reduce` resolutions down (made at the first use of that `reduce`, kept in the plan); the refusals of
// include/j2kgfx.h: J2K_ERR_UNSUPPORTED on any other plan, J2K_ERR_INVALID_ARG for a `reduce` the geometry does not allow
int plan_reduced(j2k_plan *P, int reduce, j2k::ReducedTab **out);
void free_layer_tabs(j2k_plan *P);           // j2k_layers.cpp
// a device buffer of a first-use table set: allocated if nothing failed before it (r carries the first failure; at least 64 bytes)
static inline void first_use_alloc(j2k_ctx *ctx, int &r, void **p, size_t bytes, const char *what) {
    if (r != J2K_OK) return;
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 64));
    if (e != hipSuccess) r = fail_hip(ctx, e, what);
}
// the closed-loop frame codec's tables and workspaces, made at first use (j2k_frame.cpp)
int cl_prepare(j2k_plan *P);
int cl_workspaces(j2k_plan *P);
struct ClRate { uint32_t *rate; uint64_t *dist; uint8_t *kept; uint64_t *chosen; uint8_t *floors, *floors_r; double *achieved; uint64_t *spmask; };   // chosen, achieved: 32 x F words, [layer][frame of the batch]
int cl_rate_workspace(j2k_plan *P, ClRate &W, bool passes = false);    // passes: rate / dist are the 96-entry pass tables (their own allocation), spmask beside them
int layer_tab(j2k_plan *P, int L, j2k::LayerTab **out);     // the tables of layer count L, made at its first use (j2k_layers.cpp)

// ---- the closed-loop frame codec: one encoder, one decoder (j2k_frame.cpp) ----
// How a frame's blocks are cut.  NONE: every block whole.  BYTES: the cumulative budgets[0 .. nlayers) of body bytes.  DISTORTION: the falling
// targets[0 .. nlayers) of weighted distortion, d_achieved (device, or null) = what every layer's choice reached.  layered: the layer-major
// stream with its layer ends (else nlayers = 1 and the kept-prefix stream of the _rate calls).  roi (or null): the rectangle whose footprint
// counts roi_gain times in the distortion tables.
struct EncodeRequest {
    enum Kind { NONE, BYTES, DISTORTION } kind = NONE;
    int nlayers = 1;
    bool layered = false;
    uint64_t budgets[J2K_MAX_LAYERS] = {};
    double targets[J2K_MAX_LAYERS] = {};
    const j2k_rect *roi = nullptr;
    int roi_gain = 1;
    double *d_achieved = nullptr;
    bool passes = false;      // the blocks are cut at coding-pass ends (the _passes calls: one budget or one target, no layers, no roi)
    // a batch plan with j2k_plan_set_rate_per_frame (rate_frames(P) = F frames): every frame is cut alone under budgets / targets; per_frame (the
    // _frames calls; one layer, no roi): under ITS entry of frame_values (F budgets, or the bits of F float64 targets) -- d_achieved: F per layer
    bool per_frame = false;
    std::vector<uint64_t> frame_values;
};
// an entry point's arguments -> its request, or the refusal (through fail(), naming `who`), in this order: the plan (rate_check), the layer count,
// the rectangle and gain (check_roi), the budgets or targets (targets != NULL: DISTORTION), more than one of them without the layered stream
int encode_request(j2k_plan *P, const char *who, const int64_t *layer_bytes, const double *targets, int nlayers, bool layered, bool check_roi, const j2k_rect *roi,
                   int roi_gain, double *d_achieved, EncodeRequest &q);
int layers_check(j2k_plan *P, int nlayers, const char *who);     // what every layer call needs: the plan rate_check accepts, a layer count 1 ... 32 (j2k_layers.cpp)
// coefficients -> tile-parts, THE stage order of every encode form: block coding into the plan's slots (with the rate / distortion tables unless
// NONE), the allocation, the packets of the kept-prefix or of the layered stream (d_layer_offs: its layer ends).  d_lens / d_numbps: the caller's
// tables, filled with the UNCUT lengths and plane counts.  The callers have checked the request.
int plan_encode_frame_from_coeff(j2k_plan *P, const int32_t *d_coeff, uint32_t *d_lens, uint8_t *d_numbps, const EncodeRequest &q, int sop, int eph, uint8_t *d_out,
                                 size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs);
// ... from whatever `forward` puts into the plan's closed-loop coefficient buffer (its argument), with that set's tables
int plan_encode_frame_cl(j2k_plan *P, const EncodeRequest &q, const std::function<int(int32_t *)> &forward, int sop, int eph, uint8_t *d_out, size_t cap,
                         uint64_t *d_tile_offs, uint64_t *d_layer_offs);
// What a frame decode reads and how far: layers > 0: the first `layers` layers of a layered stream; truncated: a kept-prefix stream (per-block
// floors); reduce: resolutions left out (Mallat plans); skip_planes: the uniform quality floor; area (or null): only that rectangle.
// passes (with truncated): the header's pass count is read at pass granularity and every block takes the pass-cut decode kernel.
struct DecodeRequest { int layers = 0; bool truncated = false; int reduce = 0, skip_planes = 0; const j2k_rect *area = nullptr; bool passes = false; };
struct AreaOut { int x0, y0, w, h; };      // the rectangle of the reduced frame an area call returns (j2k_area.cpp: area_check)
int area_check(const j2k_plan *P, const j2k_rect *area, int reduce, AreaOut &out, const char *who);     // every refusal a rectangle and its plan decide (host only)
// tile-parts -> pixels, THE stage order of every decode form: parse, need set, block decode + placement, inverse transform.  out: area != NULL.
// The callers have checked the request; refuses a `reduce` the plan does not allow, null d_cs / d_pix, and first use while capturing.
int plan_decode_frame(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, const DecodeRequest &q, const AreaOut *out, void *d_pix,
                      size_t stride);
int area_launch(j2k_plan *P, const j2k_rect *area, int reduce, uint8_t *d_need, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors);   // j2k_area.cpp
int decode_tile_parts_layers_launch(j2k_plan *P, j2k::LayerTab &T, int layers, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                    uint8_t *d_dense, size_t dense_cap, uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors);   // j2k_layers.cpp
int encode_tile_parts_layers_launch(j2k_plan *P, j2k::LayerTab &T, int L, const uint8_t *d_data, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                    const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                    uint64_t *d_layer_offs);   // j2k_layers.cpp
// ---- host memory in, host memory out (j2k_hostcalls.cpp) ----
int host_call_check(j2k_plan *P, const void *in, const void *out);   // J2K_ERR_INVALID_ARG for a null one; the refusal of a synchronising call while the context captures
int pix_format_bytes(int format);                                    // bytes per pixel of a J2K_PIX_* format, 0 for anything else
// THE host encode driver: `forward` (host image -> device -> forward transform into the buffer it is given), the one encoder, offsets / lens /
// numbps / achieved back, synchronise, fault and status, then the tile-parts at their exact length.  cl_set: the plan's closed-loop buffers
// (the layered, roi and quality forms), else P->d_coeff / d_lens / d_numbps; bound: what d_host_io holds of tile-parts, and the device call's cap
int encode_host(j2k_plan *P, const EncodeRequest &q, bool cl_set, size_t bound, int sop, int eph, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs,
                uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps, double *achieved, const std::function<int(int32_t *)> &forward);
// ... its launch half, shared with the pipelined form (j2k_pipe.cpp): the plan's workspaces, `forward`, the one encoder (or the reference-mode
// branch) writing the tile-parts and, behind them, their offsets into d_io (encode_host_io_bytes of device memory).  Nothing is copied back and
// nothing synchronises once the plan's workspaces exist.  io: where the results lie on the device -- offs_count words at d_offs belong at
// entry offs_at of the host's table [tile offsets (tiles + 1) | layer ends (nl)]; reference mode: the one length word, entry `tiles`
struct HostEncodeIO {
    EncodeRequest q;
    size_t nl = 0, offs_at = 0, offs_count = 0;
    const uint64_t *d_offs = nullptr;
    const uint32_t *d_lens = nullptr;
    const uint8_t *d_numbps = nullptr;
};
size_t encode_host_io_bytes(const j2k_plan *P, bool cl_set, int nlayers, size_t bound);
int encode_host_launch(j2k_plan *P, const EncodeRequest &q, bool cl_set, size_t bound, int sop, int eph, void *d_io, const std::function<int(int32_t *)> &forward,
                       HostEncodeIO &io);
size_t plain_bound(const j2k_plan *P);      // `bound` of the plain forms: j2k_plan_frame_bound (closed loop) / j2k_plan_tile_parts_bound
// reference mode: where tile-part t starts, from the dense stream's block offsets boffs (blocks + 1) -- 14 t bytes behind its tile's first block
void reference_tile_offs(const j2k_plan *P, const uint64_t *boffs, size_t total, uint64_t *tile_offs);
int frame_status_result(j2k_ctx *ctx, int st);      // a value of the frame status word -> what j2k_plan_frame_status returns for it (j2k_frame.cpp)
int fault_result(j2k_ctx *ctx, int f);              // a value of the block coders' fault word -> what check_fault returns for it (j2k_ctx.cpp)
// ... for image.*.Pix in host memory: the format / stride refusal, the pixels' staging buffer, the H2D copy and j2k_plan_forward_pixels as `forward`
int encode_pixels_host(j2k_plan *P, int format, const void *pix, size_t stride, const EncodeRequest &q, bool cl_set, size_t bound, int sop, int eph, uint8_t *out,
                       size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps, double *achieved);
// THE host decode driver: H2D, `decode` (a device frame decode of d_host_io into d_host_pix), D2H of pixbytes, the frame status; status_first
// (the area call): the status is read before the copy back, so that a refused stream leaves pix alone
int decode_host(j2k_plan *P, const uint8_t *cs, size_t len, size_t pixbytes, void *pix, bool status_first, const std::function<int(const uint8_t *, void *)> &decode);
static inline size_t reduced_rows(int H, int reduce) { return reduce > 0 ? (size_t)(((int64_t)H + (((int64_t)1 << reduce) - 1)) >> reduce) : (size_t)H; }
int rate_check(j2k_plan *P, const char *who);    // what every rate call needs of its plan (j2k_rate.cpp)
int raw_magref_refuse(const j2k_plan *P, const char *who);    // J2K_ERR_UNSUPPORTED on a plan in the raw-MagRef style (j2k_stages.cpp): the calls that cut bodies or read cut ones
int rate_upload_weights(j2k_plan *P);            // the per-job weights, the allocation workspace and (rate_per_frame) the frame ranges on the device (j2k_rate.cpp)
int rate_frames(const j2k_plan *P);              // F: the frames a rate call allocates separately -- height / frame_rows with j2k_plan_set_rate_per_frame, else 1
// the one allocation launch of a request on its tables (the frame encoder; the stage calls go through it too): kind, layers, passes, per_frame
int rate_allocate_launch(j2k_plan *P, const EncodeRequest &q, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, uint8_t *d_kept,
                         uint64_t *d_chosen, double *d_achieved);
// the _frames calls' vector: nframes == F, no negative budget / no target that is not finite or is negative -> q.per_frame, q.frame_values
int frame_values_request(j2k_plan *P, const char *who, const int64_t *frame_bytes, const double *frame_targets, int nframes, EncodeRequest &q);
int targets_check(j2k_ctx *ctx, const double *targets, int nlayers, const char *who);   // distortion targets: finite, >= 0, none above the one before (j2k_rate.cpp)
// the plan data of area_blocks_kernel (and of the region-of-interest kernels), uploaded at first use; frame: also the staging frame of a region
// decode (j2k_area.cpp)
int area_tables(j2k_plan *P, bool frame);
// region-of-interest encode (j2k_rate.cpp).  roi_check: every refusal its plan, rectangle and gain decide (host only; after rate_check).
// plan_encode_blocks_planes_roi: j2k_plan_encode_blocks_planes with the rectangle's footprint weighted roi_gain times in d_dist; roi == NULL is
// that call itself.  The callers have checked.
int roi_check(j2k_plan *P, const j2k_rect *roi, int roi_gain, const char *who);
int plan_encode_blocks_planes_roi(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate, uint64_t *d_dist,
                                  const j2k_rect *roi, int roi_gain);

// ---- stages (j2k_stages.cpp) ----
struct T1Workspace { size_t off_nsyms, off_sym, stride, total; };
T1Workspace t1_workspace(const j2k_ctx *ctx, size_t n, size_t wpj);
int ensure(j2k_ctx *ctx, void **p, size_t bytes);
int ensure_sized(j2k_plan *P, void **p, size_t *cur, size_t need);   // a buffer of the plan that grows (synchronises and bumps the plan's generation when it does; j2k_hostcalls.cpp)
struct PixIO { int stride = 0, single = 0, triple = 0; j2k::YccSrc ycc{}; };   // ycc.y: a YCbCr image in place of packed RGBA8 (triple 8)
int plan_forward_impl(j2k_plan *P, const void *d_frame, void *d_coeff, PixIO pix = PixIO());
int plan_encode_blocks_impl(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate, uint64_t *d_spmask = nullptr);
// j2k_plan_encode_blocks_passes without its checks (j2k_passes.cpp): the pass tables of every block
int plan_encode_blocks_passes(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate, uint64_t *d_dist, uint64_t *d_spmask);
// the packets of a frame written where they end up (j2k_frame.cpp); d_kept + d_rate: every block cut; passes: at coding-pass ends (96-entry tables)
int encode_tile_parts_impl(j2k_plan *P, const uint8_t *d_data, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps, int sop, int eph, uint8_t *d_out,
                           size_t cap, uint64_t *d_tile_offs, const uint8_t *d_kept = nullptr, const uint32_t *d_rate = nullptr, int passes = 0);
int decode_tile_parts_impl(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, uint64_t *d_offs, uint32_t *d_lens,
                           uint8_t *d_numbps, uint8_t *d_floors, uint8_t *d_pfloors = nullptr);
int plan_encode_private_slots(j2k_plan *P, const int32_t *d_coeff, uint32_t *d_lens, uint8_t *d_numbps);
// guard (device, or null): the launches that write d_frame write nothing if *guard != 0 -- the frame decoder's status word
int plan_inverse_impl(j2k_plan *P, const void *d_coeff, void *d_frame, PixIO pix = PixIO(), const int *guard = nullptr);
int plan_inverse_pixels_impl(j2k_plan *P, const int32_t *d_coeff, void *d_pix, size_t stride, const int *guard);
int plan_inverse_pixels_reduced_impl(j2k_plan *P, const int32_t *d_coeff, int reduce, void *d_pix, size_t stride, const int *guard);
// j2k_plan_decode_blocks on a job table of its own (the plan's, or the subset of a reduced-resolution decode); placed != NULL (HT): every block
// straight into its window of the coefficient planes `d_decoded`, coded rows only.  skip_planes: the quality floor of the _coarse calls (MQ coder;
// the callers have checked its range and the coder)
int plan_decode_blocks_jobs(j2k_plan *P, const j2k::BlockJob *d_djobs, int n, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                            const uint8_t *d_numbps, int32_t *d_decoded, const j2k::BlockJob *d_placed, int skip_planes = 0, const uint8_t *d_floors = nullptr,
                            const uint8_t *d_pfloors = nullptr);     // d_pfloors (MQ plans the rate calls accept): floors in coding passes, every block on the one-launch kernel
// the range of skip_planes and the coder it needs: J2K_OK, or the refusal (through fail())
int check_skip_planes(j2k_ctx *ctx, int coder, int skip_planes, const char *who);
// the default branch of extractImageData (j2k_image.cpp): d_img's planes on the device; status_word non-null = report a palette index
// >= npal there (the frame codec's status, asynchronous), else synchronise and return J2K_ERR_GO_PANIC before anything is written
bool plan_rgba8_wg_fusable(const j2k_plan *P);
int plan_forward_image_impl(j2k_plan *P, const j2k_image *d_img, int32_t *d_coeff, int *status_word);
int image_device_bytes(const j2k_image *img, uint64_t need[3]);
size_t image_layout(const j2k_image *img, const uint64_t need[3], size_t off[4]);
int image_upload(j2k_ctx *ctx, const j2k_image *img, const uint64_t need[3], uint8_t *dev, const size_t off[4], j2k_image *d_img);
