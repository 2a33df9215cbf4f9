/*
 * j2kgfx.h -- C ABI of libj2kgfx.so: the MI355X (gfx950) implementation of the
 * go-jpeg2000 tile-component hot path (DC shift -> MCT -> multi-level DWT ->
 * code-block entropy coding, and the inverse).
 *
 * This is the drop-in boundary.  Every entry point names the
 * reference function (file:line in mrjoshuak/go-jpeg2000) whose body a cgo shim
 * would replace with it; INTEGRATION.md shows the Go side.  Plain pointers and
 * sizes only.  All functions return J2K_OK (0) or a negative status; none abort.
 *
 * Two families:
 *   1. "host" calls -- caller-owned HOST buffers, mutated in place exactly like
 *      the Go slices they stand for; synchronous (H2D, kernels, D2H inside).
 *      One call per reference function, for unit parity and for the cgo shim.
 *   2. "plan" calls -- a frame geometry compiled once into device job tables;
 *      DEVICE pointers, asynchronous on the context's HIP stream.  This is the
 *      batched, tile-component-granular path the encoder/decoder drivers use
 *      (per-call cgo + PCIe cost forbids per-block calls).
 *
 * There is no CPU fallback: without a usable HIP device every compute call
 * returns J2K_ERR_NO_DEVICE.
 */
#ifndef J2KGFX_H
#define J2KGFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define J2K_OK 0
#define J2K_ERR_INVALID_ARG (-1)
#define J2K_ERR_NO_DEVICE (-2)
#define J2K_ERR_HIP (-3)
#define J2K_ERR_CAPACITY (-4)     /* caller's output buffer too small */
#define J2K_ERR_GO_PANIC (-5)     /* input on which the reference itself panics / never returns */
#define J2K_ERR_UNSUPPORTED (-6)

/* entropy.BandLL..BandHH (internal/entropy/t1.go:125-130) */
#define J2K_BAND_LL 0
#define J2K_BAND_HL 1
#define J2K_BAND_LH 2
#define J2K_BAND_HH 3

#define J2K_CODER_MQ 0            /* entropy.T1 (EncodeFast5 / Decode)          */
#define J2K_CODER_HT 1            /* entropy.HTEncoder / HTDecoder (bug for bug) */

typedef struct j2k_ctx j2k_ctx;   /* one HIP device + one stream + workspaces; single-threaded */
typedef struct j2k_plan j2k_plan; /* frame geometry compiled to device job tables */

/* ---- context --------------------------------------------------------------- */
int j2k_ctx_create(int device, j2k_ctx **out);
void j2k_ctx_destroy(j2k_ctx *ctx);
int j2k_ctx_sync(j2k_ctx *ctx);                 /* hipStreamSynchronize on the ctx stream */
void *j2k_ctx_stream(j2k_ctx *ctx);             /* the hipStream_t, for event timing / interop */
const char *j2k_ctx_last_error(j2k_ctx *ctx);   /* text of the last non-OK status */
const char *j2k_status_string(int status);
const char *j2k_version(void);
/* Tuning options: which of its measured kernel forms a context takes (the defaults are what the benchmarks measured best; results
 * are identical under every setting -- tests/test_gpu_knobs.py).  Set BEFORE plans are created on the context.  Names (csrc/j2k_ctx.cpp,
 * ctx_options): "t1_dec_split" (MQ decode plane by plane from this many blocks on; -1 automatic), "t1_lanes", "t1_dec_lanes",
 * "t1_sym_mb" (cap of the MQ encoder's symbol workspace, MiB), "pix_fuse", "l0_wg", "l0_wg_inv", "l0_fuse", "plane_wg", "deep", "mega",
 * "ht_dec_front" (3 | 1), "ht_dec_lean" (0 | 1), "ht_dec_dedup" (0 | 1, default 1: HT block decode skips a job whose bytes equal its leader's,
 * j2k_plan_get_ht_decode_leaders), ...  An unknown name or a value out of range is J2K_ERR_INVALID_ARG.  The ENVIRONMENT sets none of this unless J2K_TUNING=1 is in
 * it (then J2K_<NAME> is read for every option at j2k_ctx_create: the tests' and tools' A/B switch); J2K_RCCL_LIB, the path of the
 * RCCL library, is the one variable that is always read. */
int j2k_ctx_set_option(j2k_ctx *ctx, const char *name, long value);
/* Kernel timing for bench.py's roofline lines: while enabled, the dispatches of the 5-3 transform stamp a HIP event pair
 * with the kernel's own begin and end (hipExtLaunchKernelGGL start/stop events on the ctx stream).  on = 1: the level-0
 * dispatch of every j2k_plan_forward* only (tag 0; cheapest, used inside bench.py's timed region); on = 2: every
 * dispatch of j2k_plan_forward* and j2k_plan_inverse*, tagged 0 = forward level 0, 1 = forward deeper levels, 2 = inverse
 * level 0, 3 = inverse deeper levels.  j2k_ctx_profile_read_tag synchronises and returns the number of recorded dispatches
 * with that tag and their summed duration in ms; j2k_ctx_profile_read does the same for tag 0 and resets the counters. */
int j2k_ctx_profile_enable(j2k_ctx *ctx, int on);
int j2k_ctx_profile_read(j2k_ctx *ctx, int64_t *launches, double *total_ms);
int j2k_ctx_profile_read_tag(j2k_ctx *ctx, int tag, int64_t *launches, double *total_ms);

/* HIP graphs (no counterpart in the reference: a launch-overhead facility of this boundary).  Between
 * capture_begin and capture_end the asynchronous device-pointer calls of this context (section 2: j2k_plan_forward*,
 * j2k_plan_encode_stream, j2k_plan_decode_blocks, j2k_plan_inverse*, j2k_plan_assemble_tiles_device ...) are recorded
 * instead of run; j2k_graph_launch replays them on the context's stream with the same device pointers (new contents in
 * the same buffers).  The same calls must have run once before the capture (workspaces sized): a call that would have to
 * allocate fails with J2K_ERR_INVALID_ARG and the capture must be ended and discarded.  Synchronous calls (anything in
 * section 1, j2k_ctx_sync, j2k_ctx_profile_read) are not allowed while capturing.
 *
 * LIFETIME.  Besides the caller's own buffers (which the caller keeps alive and in place) a graph records device memory of the library:
 * the context's staging workspaces that the recorded calls reserved, and the tables and workspaces of the plans whose calls were recorded.
 * A graph is STALE once, since its capture_end,
 *   (a) a staging workspace of its context that the capture used was reallocated -- a later call on the SAME CONTEXT, from any of its plans or
 *       a call that was not captured, needed it larger (a larger frame, more blocks);
 *   (b) a growable buffer of a plan whose calls the capture recorded was reallocated -- j2k_plan_decode_frame_pixels_layers / _area with layers
 *       on a longer stream than any before, or a host call (section 1 forms: j2k_encode_pixels_host*, j2k_decode_pixels_host*) of that plan at
 *       a larger size;
 *   (c) such a plan was destroyed.
 * j2k_graph_launch on a stale graph returns J2K_ERR_INVALID_ARG, j2k_ctx_last_error names (a), (b) or (c); nothing is launched and the context
 * stays usable.  j2k_graph_stale returns 0 for a valid graph and 1 / 2 / 3 for (a) / (b) / (c) (0 for NULL).  j2k_graph_destroy of a stale graph
 * is legal; after one ordinary (warm) run of the same calls a new capture gives a valid graph again.  Nothing else stales a graph: not the
 * growth of a workspace the capture did not use, not the growth or the destruction of a plan it did not call, nothing on another context.
 * Plans are noted at every j2k_plan_* entry point that takes a non-const plan, so no call family relies on the conservative alternative
 * ("every plan alive at capture_end").  The buffers of a j2k_pipe are never recorded: j2k_pipe_create and both submits refuse while the
 * context captures.  A graph must be destroyed before its context. */
typedef struct j2k_graph j2k_graph;
int j2k_ctx_capture_begin(j2k_ctx *ctx);
int j2k_ctx_capture_end(j2k_ctx *ctx, j2k_graph **out);
int j2k_graph_launch(j2k_graph *g);
int j2k_graph_stale(const j2k_graph *g);
void j2k_graph_destroy(j2k_graph *g);

/* ==== 1. host calls: one per reference function ============================= */

/* mct.DCLevelShiftForward / Inverse   (internal/mct/mct.go:96-101, 113-118) */
int j2k_dc_level_shift_forward(j2k_ctx *ctx, int32_t *data, size_t n, int precision);
int j2k_dc_level_shift_inverse(j2k_ctx *ctx, int32_t *data, size_t n, int precision);
/* mct.ForwardRCT / InverseRCT         (mct.go:28-38, 56-66) */
int j2k_forward_rct(j2k_ctx *ctx, int32_t *r, int32_t *g, int32_t *b, size_t n);
int j2k_inverse_rct(j2k_ctx *ctx, int32_t *y, int32_t *u, int32_t *v, size_t n);
/* mct.ForwardICT / InverseICT         (mct.go:14-24, 43-53) */
int j2k_forward_ict(j2k_ctx *ctx, double *r, double *g, double *b, size_t n);
int j2k_inverse_ict(j2k_ctx *ctx, double *y, double *cb, double *cr, size_t n);

/* dwt.Forward53 / Inverse53 (1-D)     (internal/dwt/dwt.go:73-118, 122-147) */
int j2k_forward53(j2k_ctx *ctx, int32_t *data, int length);
int j2k_inverse53(j2k_ctx *ctx, int32_t *data, int length);
/* dwt.Forward97 / Inverse97 (1-D)     (dwt.go:161-210, 213-262) */
int j2k_forward97(j2k_ctx *ctx, double *data, int length);
int j2k_inverse97(j2k_ctx *ctx, double *data, int length);
/* dwt.Forward2D53 / Inverse2D53 / Forward2D97 / Inverse2D97 (dwt.go:356-473) */
int j2k_forward2d53(j2k_ctx *ctx, int32_t *data, int width, int height);
int j2k_inverse2d53(j2k_ctx *ctx, int32_t *data, int width, int height);
int j2k_forward2d97(j2k_ctx *ctx, double *data, int width, int height);
int j2k_inverse2d97(j2k_ctx *ctx, double *data, int width, int height);
/* dwt.DecomposeMultiLevel53/97, ReconstructMultiLevel53/97 (dwt.go:524-573);
 * the reference's contiguous-prefix level layout is reproduced exactly. */
int j2k_decompose_multilevel53(j2k_ctx *ctx, int32_t *data, int width, int height, int levels);
int j2k_reconstruct_multilevel53(j2k_ctx *ctx, int32_t *data, int width, int height, int levels);
int j2k_decompose_multilevel97(j2k_ctx *ctx, double *data, int width, int height, int levels);
int j2k_reconstruct_multilevel97(j2k_ctx *ctx, double *data, int width, int height, int levels);

/* dwt.Quantize (dwt.go:500-511): invStep = 1.0 / step_size, then int32(math.Floor(v*invStep + 0.5)) for v >= 0 (-0.0 included),
 * int32(math.Ceil(v*invStep - 0.5)) otherwise; int32() as Go converts (out of range and NaN: 0x80000000).  NOT the encoder's
 * quantiser (encoder.go:270-275 divides and truncates).  dwt.Dequantize (dwt.go:514-520): float64(v) * step_size.  n == 0: no-op. */
int j2k_quantize(j2k_ctx *ctx, const double *src, size_t n, double step_size, int32_t *dst);
int j2k_dequantize(j2k_ctx *ctx, const int32_t *src, size_t n, double step_size, double *dst);

/* tcd.TileEncoder.ApplyForwardDWT / TileDecoder.ApplyInverseDWT on one
 * tile-component (internal/tcd/tcd.go:508-534, 416-437): reversible -> 5-3 int32;
 * else int32->f64, 9-7, int32(v +- 0.5) forward / int32(v + 0.5) inverse. */
int j2k_tcd_apply_forward_dwt(j2k_ctx *ctx, int32_t *data, int width, int height, int levels, int reversible);
int j2k_tcd_apply_inverse_dwt(j2k_ctx *ctx, int32_t *data, int width, int height, int levels, int reversible);

/* One code-block job of a batch.  For encode: the window (x0,y0,w,h) of plane
 * `plane` (stride = that plane's width) is the block, exactly what
 * encoder.extractCodeBlockData hands to T1.SetData (encoder.go:763-795).
 * For decode: bytes [in_off, in_off+in_len) of the input stream, numbps, band. */
typedef struct {
    int32_t plane;      /* index into the planes[] array of the call */
    int32_t band;       /* J2K_BAND_* */
    int32_t x0, y0;     /* window origin in the plane */
    int32_t w, h;       /* block size (actualWidth, actualHeight) */
} j2k_block;

/* entropy.(*T1).SetData + Encode(band) (t1.go:292-304, t1_fast5.go:10-899) or
 * entropy.(*HTEncoder).SetData + Encode(band) (ht.go:935-1045) for n blocks.
 * planes[i] is a HOST int32 plane of plane_w[i] x plane_h[i].  Output: block j's
 * bytes at out[offs[j] .. offs[j]+lens[j]) in job order (lens[j]==0 <=> Go nil),
 * numbps[j] = bit length of max |x| (the value T1.Decode must be told). */
int j2k_encode_blocks(j2k_ctx *ctx, int coder, const int32_t *const *planes, const int32_t *plane_w,
                      const int32_t *plane_h, int nplanes, const j2k_block *blocks, size_t nblocks,
                      uint8_t *out, size_t cap, uint64_t *offs, uint32_t *lens, uint8_t *numbps,
                      size_t *total);
/* entropy.NewT1(w,h).Decode(bytes,numBPS,band) (t1.go:1261-1292) or a fresh
 * entropy.NewHTDecoder(w,h).Decode(bytes,numBitplanes,band) (ht.go:93-150) for n
 * blocks.  Block j's coefficients (w*h int32, dense) land at coeffs + coeff_offs[j]. */
int j2k_decode_blocks(j2k_ctx *ctx, int coder, const uint8_t *bytes, const uint64_t *offs,
                      const uint32_t *lens, const uint8_t *numbps, const j2k_block *blocks,
                      size_t nblocks, int32_t *coeffs, const uint64_t *coeff_offs);
/* Quality-scalable T1.Decode (MQ coder; a feature of this library, the reference decodes every block to its last plane):
 * skip_planes = k, 0 ... 31.  Every block's loop `for bp = numBPS-1 ... 0` (t1.go:1261-1410) runs down to plane k only -- all three
 * passes of a plane or none; a block with numBPS <= k reads nothing of its stream and is zeros -- and every non-zero magnitude
 * takes the midpoint of the planes left undecoded (bit k-1, for k >= 1) before its sign.  With v the sample of the full decode,
 * |v| < 2^31:   m = |v| & ~(2^k - 1);  result = sign(v) * (m != 0 && k >= 1 ? m | 2^(k-1) : m).
 * k = 0 is j2k_decode_blocks; k outside 0 ... 31: J2K_ERR_INVALID_ARG; k > 0 with J2K_CODER_HT: J2K_ERR_UNSUPPORTED (its one
 * pass has no planes to stop between).  The same argument in j2k_plan_decode_blocks_coarse, j2k_plan_decode_frame_pixels_coarse
 * and j2k_decode_pixels_host_coarse below. */
int j2k_decode_blocks_coarse(j2k_ctx *ctx, int coder, const uint8_t *bytes, const uint64_t *offs,
                             const uint32_t *lens, const uint8_t *numbps, const j2k_block *blocks,
                             size_t nblocks, int skip_planes, int32_t *coeffs, const uint64_t *coeff_offs);
/* worst-case bytes one w x h block can produce (sizing of `out`) */
size_t j2k_block_bound(int coder, int w, int h);

/* ==== 2. plan calls: batched frame pipeline on device buffers ================ */

typedef struct {
    int32_t width, height;      /* frame size in samples                                     */
    int32_t ncomp;              /* components; planar int32 [C][H][W] (encoder.componentData) */
    int32_t precision;          /* bits per sample -> DC shift 1<<(p-1)  (encoder.go:218-220) */
    int32_t is_signed;          /* decode: skip DC shift for signed comps (decoder.go:344-348) */
    int32_t lossless;           /* 1: RCT + 5-3 ; 0: ICT + 9-7 + quantise (encoder.go:223-277) */
    int32_t quality;            /* Options.Quality, <=0 -> 100 (encoder.go:265-269)           */
    int32_t num_resolutions;    /* Options.NumResolutions; levels = n-1, <=0 -> 5; jobs: <=0 -> 6 */
    int32_t cb_w, cb_h;         /* REAL code-block size, 1<<(CodeBlockSize+2) (encoder.go:606-613) */
    int32_t tile_w, tile_h;     /* 0 = one tile (the reference); else tile t == the reference
                                   pipeline run on the cropped sub-image          */
    int32_t coder;              /* J2K_CODER_MQ | J2K_CODER_HT                                */
    int32_t tile_first, tile_count; /* shard: tiles [first, first+count); count<=0 -> all     */
    int32_t frame_rows;         /* > 0: a BATCH -- height / frame_rows frames of `width` x frame_rows stacked
                                   vertically (planes [C][height][W], pixels height rows): the tile grid starts
                                   again at every frame, so every frame is coded exactly as it would be alone,
                                   and one call carries all of them in its launches (tiles are numbered frame
                                   after frame).  0: one frame of `height` rows.  height % frame_rows must be 0 */
    int32_t closed_loop;        /* 0 (default): the reference's behaviour, byte for byte -- code-block windows cut from the
                                   top left of the plane for every band (encoder.go:763-795: they overlap, most of the
                                   plane is never coded) and Tier-2 packets that the reference's own decoder cannot read.
                                   1: THIS LIBRARY'S closed-loop mode, outside reference parity (SURVEY 8f rank 3 asks for
                                   "proper sub-band addressing and a real decode body"): band b of resolution r is the
                                   Mallat rectangle of decomposition level l = numRes-1-r of the tile-component
                                   (w_0 = w, w_{l+1} = ceil(w_l/2); LL = [0,w_L) x [0,h_L), HL = [w_{l+1},w_l) x [0,h_{l+1}),
                                   LH = [0,w_{l+1}) x [h_{l+1},h_l), HH the rest), cut into cb_w x cb_h blocks from the
                                   band's origin: the windows PARTITION the plane, job order stays comp -> res -> band ->
                                   row -> column, and j2k_plan_encode_tile_parts / j2k_plan_decode_tile_parts write and
                                   read packets with the J2K_T2_* flags below, so that pixels -> tile-parts -> pixels is
                                   a bit-exact round trip with the MQ coder.  Transform, block coders and every byte of
                                   a code-block are the reference's in both modes.
                                   2 (J2K_CLOSED_LOOP_MALLAT): the closed-loop mode with a Mallat decomposition under it, also
                                   outside reference parity.  In modes 0 and 1 level l+1 of the transform runs on the first
                                   w_{l+1} h_{l+1} LINEAR elements of the plane (dwt.DecomposeMultiLevel53/97, dwt.go:524-573):
                                   only level 0 decorrelates the picture and the rectangles above are labels, not sub-bands.
                                   Here level l is the reference's single-level 2-D transform (Forward2D53 / Forward2D97,
                                   dwt.go:356-473) on the RECTANGLE [0,w_l) x [0,h_l) of the plane, read as a dense w_l x h_l
                                   matrix and written back in place (row stride = the plane's width); the inverse walks the
                                   levels back the same way.  DC shift, RCT / ICT and its rounding, the float64 plane kept
                                   across all 9-7 levels, the quantiser, int32(v + 0.5), j2k_plan_set_dequantize, the windows,
                                   job order, block coders, packets, tile-parts, batches and shards are those of mode 1 --
                                   the windows now ARE the sub-bands of each resolution, streams are smaller, and
                                   LL_r is a picture: the j2k_plan_*_reduced calls below.  Lossless plans have, at level 0,
                                   the packed-RGBA8 workgroup form and single-component planes in workgroup form, where
                                   the geometry admits them (the prefix contracts; they imply tiles a multiple of 8 wide):
                                   the *_pixels calls then read / write the pixels in the level-0 launch, and
                                   j2k_plan_pixels_fused reports 1, wherever a plan of modes 0 / 1 would AND that launch
                                   is one of these workgroup forms -- RGBA8 without its workgroup table and Gray16 without
                                   the plane table keep the int32 staging frame (report 0).  Every level below level 0 is
                                   one launch of the general kernels.  Not built: the tail / deep / merged / fused-level
                                   launches and the plane form below level 0, the 9-7 workgroup forms, image sources read
                                   directly, pixel fusion of a reduced decode's final launch.
                                   The streams are still not Part-1 conformant: the packet headers are the reference's */
} j2k_params;
#define J2K_CLOSED_LOOP_MALLAT 2

typedef struct {
    int64_t tiles;              /* tiles in this shard                                        */
    int64_t planes;             /* tile-components                                            */
    int64_t blocks;             /* code-block jobs                                            */
    int64_t coeff_elems;        /* int32 elements of the coefficient buffer                   */
    int64_t bytes_cap;          /* bytes of the worst-case slotted block output               */
    int64_t dwt_bytes;          /* algorithmic bytes of the multi-level DWT       */
    int64_t dwt_level0_bytes;   /* algorithmic bytes of the level-0 kernel launch             */
    int64_t block_samples;      /* samples the block coder reads                              */
    int64_t decoded_elems;      /* int32 elements of the dense decoded-block buffer           */
} j2k_plan_info;

int j2k_plan_create(j2k_ctx *ctx, const j2k_params *params, j2k_plan **out);
void j2k_plan_destroy(j2k_plan *plan);
int j2k_plan_get_info(const j2k_plan *plan, j2k_plan_info *info);
/* copy out the job list (reference order: tile -> comp -> res -> band -> cby -> cbx) */
int j2k_plan_get_blocks(const j2k_plan *plan, j2k_block *blocks, size_t cap);
/* per-plane geometry: tile index, component, x0, y0, w, h, coefficient offset (7 x int64 each) */
int j2k_plan_get_planes(const j2k_plan *plan, int64_t *desc7, size_t cap_planes);

/* encoder.preprocess (encoder.go:216-281) for every tile-component of the shard:
 * d_frame = device int32 [C][H][W] pixels (read only), d_coeff = device coefficient
 * buffer (coeff_elems int32; each tile-component dense w_t x h_t at its offset). */
int j2k_plan_forward(j2k_plan *plan, const int32_t *d_frame, int32_t *d_coeff);
/* inverse path: ApplyInverseDWT per tile-component + inverse MCT + DC shift
 * (tcd.go:416-437, decoder.go:321-348): d_coeff -> d_frame (pixels). */
int j2k_plan_inverse(j2k_plan *plan, const int32_t *d_coeff, int32_t *d_frame);
/* encoder.encodeTile job loop (encoder.go:616-688), sequential semantics: every job's
 * bytes into worst-case slots of d_slots (bytes_cap), lengths into d_lens (u32 per job),
 * bit-plane counts into d_numbps (u8 per job). */
int j2k_plan_encode_blocks(j2k_plan *plan, const int32_t *d_coeff, uint8_t *d_slots,
                           uint32_t *d_lens, uint8_t *d_numbps);
/* exclusive scan of d_lens -> d_offs (u64 per job, +1 total at the end) and gather of the
 * slots into the dense stream d_stream (concatenation in job order, encoder.go:684). */
int j2k_plan_compact(j2k_plan *plan, const uint8_t *d_slots, const uint32_t *d_lens,
                     uint64_t *d_offs, uint8_t *d_stream);
/* j2k_plan_encode_blocks + j2k_plan_compact in one call: the dense stream (job order), d_offs (u64
 * per job + total), d_lens, d_numbps; the slot buffer in between is owned by the plan.  (With
 * J2K_FUSE_COMPACT=1, the HT coder and blocks up to 64x64 it is one kernel with a decoupled look-back
 * over the block lengths -- correct, but measured slower than the three kernels, so off by default.) */
int j2k_plan_encode_stream(j2k_plan *plan, const int32_t *d_coeff, uint8_t *d_stream, uint64_t *d_offs,
                           uint32_t *d_lens, uint8_t *d_numbps);
/* Transport form of a stream for the multi-GPU gather (the compressed packets go to rank 0 for codestream
 * assembly, encoder.go:568-579, 746-760).  The reference's HT block carries max(64, 2wh)/4 zero bytes of MEL segment
 * (ht.go:978, 1019) -- two thirds of a 64x64 block -- and every peer has ONE xGMI link to the root, so a peer sends
 *   header | lens u32[n] | maglens u32[n] | numbps u8[n] | offs u64[n+1] | toffs u64[n+1] | blocks without the MEL runs
 * (j2k_plan_pack_bound bytes at most; the first u64 of the pack is its length) and the root rebuilds the dense stream,
 * d_offs (n + 1), d_lens and d_numbps byte for byte with j2k_plan_unpack_stream on a plan of the same geometry (any
 * other pack is reported as J2K_ERR_INVALID_ARG at the next sync).  j2k_plan_pack_stream packs the stream made by the
 * LAST j2k_plan_encode_stream call on this plan (the plan remembers where each block's MagSgn bytes end) and returns
 * J2K_ERR_INVALID_ARG when d_stream / d_lens are not that call's outputs; MQ streams have no zero runs and are packed as
 * they are. */
size_t j2k_plan_pack_bound(const j2k_plan *plan);
int j2k_plan_pack_stream(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                         const uint8_t *d_numbps, uint8_t *d_pack);
/* pack_bytes = the bytes the caller really holds at d_pack (what it received): a pack is foreign input, and nothing
 * outside [d_pack, d_pack + pack_bytes) is read -- a pack shorter than its header is J2K_ERR_INVALID_ARG at once, one whose
 * fields point outside it or outside the stream is J2K_ERR_INVALID_ARG at the next sync and copies nothing for the
 * offending block (every bound is tested without forming a sum of untrusted 64-bit fields). */
int j2k_plan_unpack_stream(j2k_plan *plan, const uint8_t *d_pack, size_t pack_bytes, uint8_t *d_stream, uint64_t *d_offs,
                           uint32_t *d_lens, uint8_t *d_numbps);
/* the same for `count` packs of this geometry in one launch (host arrays of device pointers / of byte counts): the root
 * of an N-GPU gather rebuilds the N-1 peers' streams of a frame slot at once */
int j2k_plan_unpack_streams(j2k_plan *plan, int count, const uint8_t *const *d_packs, const size_t *pack_bytes,
                            uint8_t *const *d_streams, uint64_t *const *d_offs, uint32_t *const *d_lens, uint8_t *const *d_numbps);
/* tcd.TileDecoder.DecodeCodeBlock (tcd.go:393-413) for every job: dense stream + offsets
 * + lens + numbps -> d_decoded (decoded_elems int32, block j dense at its job offset). */
int j2k_plan_decode_blocks(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs,
                           const uint32_t *d_lens, const uint8_t *d_numbps, int32_t *d_decoded);
/* HT coder only; default off.  The reference's HT decoder writes ONE row in four of a block (ht.go:589-711: only row y of each
 * 4-row stripe is coded) and returns its internal slice: a fresh decoder's slice is zero elsewhere -- what
 * j2k_plan_decode_blocks reproduces by default, writing all w x h samples -- while a pooled decoder (GetHTDecoder /
 * PutHTDecoder, ht.go:1393-1429) is not cleared on that path and keeps whatever those rows held.  With `on` the call
 * behaves like the pooled decoder: rows y % 4 != 0 of every block in d_decoded are left untouched (the caller zeroed the
 * buffer once, or does not read them), the coded rows are written in full as before.  Three quarters of the decoder's
 * store stream (77 of 103 MB per 4K frame) disappear. */
int j2k_plan_set_decode_coded_rows_only(j2k_plan *plan, int on);
/* Lossy plans (lossless = 0) only; J2K_ERR_UNSUPPORTED otherwise.  Default off: tcd.ApplyInverseDWT as the reference
 * wrote it.  On: the inverse path multiplies every int32 coefficient by 1.0 / Quality first (dwt.Dequantize, dwt.go:514-520),
 * fused into the load of the inverse kernels.  Applies to every later call on the plan, and to what is captured into a
 * graph from then on; a graph captured earlier keeps the setting it was captured with. */
int j2k_plan_set_dequantize(j2k_plan *plan, int on);
/* The raw-MagRef coding style (this library's; the reference declares its parts -- RawEncoder / RawDecoder mqc.go:516-600, CodeBlockBypass
 * markers.go:140 -- and never connects them).  MQ plans whose code-blocks are all at most 64 x 64; J2K_ERR_UNSUPPORTED on an HT plan and on a
 * plan with a larger block; J2K_ERR_INVALID_ARG while the context captures a graph.  Default off.  On: every later block coder call of the plan
 * (j2k_plan_encode_blocks / _encode_stream / _decode_blocks / _decode_blocks_coarse, the frame calls j2k_plan_encode_frame_pixels / _image,
 * j2k_plan_decode_frame_pixels / _reduced / _coarse / _area, their host forms and captures of them) codes and reads block bodies H | MQ | RAW:
 * the decisions, their order, numBPS and every context that is not a magnitude refinement are the plain codec's; the decisions of contexts
 * Mag0 / Mag1 / Mag2 bypass the MQ coder and are written, in coding order across all planes, as one RawEncoder string RAW (MSB first, a 7-bit
 * byte after every 0xFF, Flush as written); MQ is the codeword of the remaining symbols; H = len(MQ) in three 7-bit groups, most significant
 * first.  A block without bit planes has an empty body.  Nothing above the body changes (packet headers, lens, numbps, SOP / EPH, tile-parts).
 * The decoder is a total function of (bytes, numbps): a body shorter than 3 bytes has empty MQ and RAW, len(MQ) is clamped to the body, past the
 * end of MQ the MQ decoder reads what the reference's reads, past the end of RAW and behind an 0xFF followed by a byte above 0x8F the raw reader
 * returns ones (RawDecoder.DecodeBit).  A two-stream body has no prefix property: on a plan in the style the calls that cut bodies at bit planes
 * or read cut bodies return J2K_ERR_UNSUPPORTED before anything is launched -- j2k_plan_encode_blocks_planes(_roi), every _rate / _layers / _roi /
 * _quality / _kept encode and allocation call, and the decode calls with per-block floors, truncated streams or layers.  A stream is decoded by a
 * plan with the setting it was coded with; nothing in the stream says which. */
int j2k_plan_set_raw_magref(j2k_plan *plan, int on);
/* 1 if the plan codes in the raw-MagRef style, else 0 (j2k_plan_info keeps its layout) */
int j2k_plan_get_raw_magref(const j2k_plan *plan);
/* job j's offset (in int32 elements) into d_decoded */
int j2k_plan_get_decoded_offsets(const j2k_plan *plan, uint64_t *offs, size_t cap);
/* HT plans only (J2K_ERR_UNSUPPORTED otherwise): leaders[j] = the job whose decode may serve job j as well under the context option ht_dec_dedup
 * (0 | 1, default 1; J2K_HT_DEC_DEDUP with J2K_TUNING=1) -- the lowest job with the same window of the same width and height, when the width is 8, 16,
 * 32 or 64, the block is on the parallel path, both decoded offsets are multiples of 4 and the leader has fewer than 7 followers so far; j itself
 * otherwise.  A candidate only: j2k_plan_decode_blocks compares the bytes of the two blocks in every call and decodes job j on its own unless
 * they are equal, so the option never changes a result.  It applies with ht_dec_front = 3 and ht_dec_lean = 1 (the defaults). */
int j2k_plan_get_ht_decode_leaders(const j2k_plan *plan, int32_t *leaders, size_t cap);
/* HT plans only: the order in which the walk stage of j2k_plan_decode_blocks takes the jobs under ht_dec_dedup -- order[s] = the job of slot s: the
 * *n_leaders (may be NULL) jobs with leaders[j] == j first, in ascending order, then every other job, ascending.  Like the leaders it is static and
 * never changes a result. */
int j2k_plan_get_ht_decode_walk_order(const j2k_plan *plan, int32_t *order, size_t cap, int32_t *n_leaders);

/* ---- the multi-GPU exchange -------------------------------------------------------------------------------
 * One process per GPU, each with its own j2k_ctx; a frame's tiles are sharded by j2k_params.tile_first / tile_count and coded
 * independently (no halo).  The ONE exchange step is the gather of the compressed streams to rank 0 for codestream assembly
 * -- it replaces the in-process collection of encoder.encodeTile's job results (encoder.go:690-742) when the jobs ran on other
 * GPUs: ncclAllGather of the byte counts, then inside one ncclGroupStart / ncclGroupEnd every rank != 0 ncclSend()s its
 * streams to rank 0, which posts the matching ncclRecv()s -- direct peer -> root over each peer's own xGMI link, no ring.
 * RCCL is bound at run time (dlopen), so a single-GPU host does not need it: the calls return J2K_ERR_UNSUPPORTED without it.
 *
 *   j2k_comm_get_unique_id   rank 0 makes the 128-byte RCCL id; the HOST carries it to the other ranks (the Go side: any
 *                            channel it has -- a pipe to its worker processes, a file, MPI; the Python tests: torch.distributed)
 *   j2k_comm_create          collective (every rank): ncclCommInitRank on ctx's device; the communicator owns a HIP stream
 *                            of its own for the transfers
 *   j2k_gather_streams       collective.  Rank r passes `count` device buffers d_send[f] of send_bytes[f] bytes (normally the
 *                            packs of j2k_plan_pack_stream, one per frame slot).  all_bytes: the byte counts of every rank,
 *                            rank-major (world x count), when the host already knows them (it usually does: a 16-byte
 *                            message per rank on whatever channel carried the id) -- else NULL and the call gathers them
 *                            with ncclAllGather, which costs a stream synchronisation.  producers: the contexts on whose
 *                            streams the send buffers are being produced; the transfers are ordered behind their work so
 *                            far.  On rank 0, stream f of rank r lands at d_recv + recv_offs[r * count + f] (16-byte
 *                            aligned; recv_offs has world * count + 1 entries, host memory, filled on every rank), its own
 *                            streams by a device copy.  Returns once the transfers are QUEUED on the communicator's
 *                            stream.  FAILURE IS COLLECTIVE where the call can make it so: J2K_ERR_CAPACITY (recv_cap of
 *                            rank 0 too small) is returned by EVERY rank when the counts are gathered by the call (rank 0's
 *                            recv_cap travels with them); with host-provided counts a peer passes rank 0's capacity as its
 *                            own recv_cap (0 = not known: that peer returns J2K_OK).  Either way nobody is left waiting:
 *                            the peers always post their sends, and a rank 0 that cannot take the bytes (too small, NULL
 *                            or misaligned d_recv) receives them into a scratch allocation, drains its stream and then
 *                            returns the status; the communicator stays usable.  Argument errors that only ONE rank can
 *                            see (J2K_ERR_INVALID_ARG: a NULL send pointer, all_bytes that disagrees with send_bytes)
 *                            return before anything is posted on that rank -- the host must agree on them before the call.
 *   j2k_comm_wait            consumer != NULL: that context's stream waits (on the device) for the last gather -- follow with
 *                            j2k_plan_unpack_streams on it; NULL: the host waits.
 * flags: J2K_GATHER_SELF_LOOP (world == 1 only): the lone rank sends to itself through RCCL -- the transfer calls on one GPU. */
typedef struct j2k_comm j2k_comm;
#define J2K_COMM_ID_BYTES 128
#define J2K_GATHER_SELF_LOOP 1
const char *j2k_comm_load_error(void);   /* why RCCL could not be bound (J2K_ERR_UNSUPPORTED); "" if it was.  J2K_RCCL_LIB names the library */
int j2k_comm_get_unique_id(uint8_t *id128);
int j2k_comm_create(j2k_ctx *ctx, const uint8_t *id128, int rank, int world, j2k_comm **out);
void j2k_comm_destroy(j2k_comm *comm);
const char *j2k_comm_last_error(j2k_comm *comm);
void *j2k_comm_stream(j2k_comm *comm);
int j2k_gather_streams(j2k_comm *comm, int count, const uint8_t *const *d_send, const uint64_t *send_bytes,
                       const uint64_t *all_bytes, j2k_ctx *const *producers, int nproducers,
                       uint8_t *d_recv, size_t recv_cap, uint64_t *recv_offs, int flags);
int j2k_comm_wait(j2k_comm *comm, j2k_ctx *consumer);

/* ---- stand-alone arithmetic / bypass coders (internal/entropy/mqc.go), host buffers ------------
 * MQEncoder: NewMQEncoder, n x Encode(ctxs[i], decisions[i]), Flush (mqc.go:169-349); *out_len = 0
 * is Flush's nil.  A context >= 19 is the Go index panic (J2K_ERR_GO_PANIC). */
int j2k_mq_encode(j2k_ctx *ctx, const uint8_t *ctxs, const uint8_t *decisions, size_t n,
                  uint8_t *out, size_t cap, size_t *out_len);
/* MQDecoder: NewMQDecoder(data), n x Decode(ctxs[i]) -> decisions[i] (mqc.go:352-497) */
int j2k_mq_decode(j2k_ctx *ctx, const uint8_t *data, size_t len, const uint8_t *ctxs, size_t n,
                  uint8_t *decisions);
/* RawEncoder: n x EncodeBit(bits[i]), Flush (mqc.go:560-600); RawDecoder: n x DecodeBit (mqc.go:516-557) */
int j2k_raw_encode(j2k_ctx *ctx, const uint8_t *bits, size_t n, uint8_t *out, size_t cap, size_t *out_len);
int j2k_raw_decode(j2k_ctx *ctx, const uint8_t *data, size_t len, size_t n, uint8_t *bits);

/* ---- pixels at native width ------------------------------------------------
 * encoder.extractImageData (encoder.go:79-213) and decoder.createImage (decoder.go:417-588): the
 * host loops on either side of the tile-component path.  Pixel buffers are Go image.* Pix layouts
 * (row-major, `stride` bytes per row, 16-bit samples big-endian). */
enum {
    J2K_PIX_GRAY8 = 0,     /* *image.Gray     1 component,  8 bit   (encoder.go:83-93)   */
    J2K_PIX_GRAY16 = 1,    /* *image.Gray16   1 component, 16 bit   (encoder.go:95-105)  */
    J2K_PIX_RGBA8 = 2,     /* *image.RGBA     3 components (alpha ignored), 8 bit (encoder.go:107-123) */
    J2K_PIX_RGBA64 = 3,    /* *image.RGBA64   3 components, 16 bit  (encoder.go:125-141) */
    J2K_PIX_NRGBA8 = 4,    /* *image.NRGBA    4 components, 8 bit   (encoder.go:143-160) */
    J2K_PIX_NRGBA64 = 5    /* *image.NRGBA64  4 components, 16 bit  (encoder.go:162-179) */
};
/* components / source precision of a pixel format (0 for an unknown format) */
int j2k_pixels_components(int format);
int j2k_pixels_precision(int format);
/* extractImageData on HOST buffers: pix -> planes[c] (ncomp planes of w*h int32, caller-allocated).
 * target_precision 1..16 applies the Options.Precision rescale (encoder.go:196-210); 0 keeps the
 * source precision.  The pixels cross PCIe at native width. */
int j2k_extract_image_data(j2k_ctx *ctx, int format, const void *pix, size_t stride, int w, int h,
                           int target_precision, int32_t *const *planes);
/* createImage on HOST buffers: planes[c] -> pix.  ncomp 1 -> Gray (precision <= 8) / Gray16;
 * 3 or 4 -> RGBA (precision <= 8) / RGBA64; other ncomp -> J2K_ERR_UNSUPPORTED (decoder.go:583-585). */
int j2k_create_image(j2k_ctx *ctx, const int32_t *const *planes, int ncomp, int precision, int w, int h,
                     void *pix, size_t stride);
/* the same on DEVICE buffers (d_planes = ncomp planes of w*h int32, contiguous) */
int j2k_unpack_pixels(j2k_ctx *ctx, int format, const void *d_pix, size_t stride, int w, int h,
                      int target_precision, int32_t *d_planes);
int j2k_pack_pixels(j2k_ctx *ctx, const int32_t *d_planes, int ncomp, int precision, int w, int h,
                    void *d_pix, size_t stride);
/* j2k_plan_forward / j2k_plan_inverse with the frame as packed 8-bit RGBA on the device
 * (extractImageData + preprocess, and the inverse path + createImage, fused): for a 3-component
 * 8-bit plan.  The 5-3 + RCT level-0 kernels read / write the pixels directly when the geometry
 * allows 16-byte accesses (otherwise the pixels pass through an int32 staging frame). */
int j2k_plan_forward_rgba8(j2k_plan *plan, const void *d_pix, size_t stride, int32_t *d_coeff);
int j2k_plan_inverse_rgba8(j2k_plan *plan, const int32_t *d_coeff, void *d_pix, size_t stride);
/* Any pixel format: extractImageData (+ the rescale to the plan's precision) then j2k_plan_forward;
 * j2k_plan_inverse then createImage for the plan's component count and precision.  The plan's
 * component count must equal j2k_pixels_components(format) (forward) / be 1, 3 or 4 (inverse).
 * When the plan's precision is the format's own (8 / 16 bit, unsigned, 5-3) and the geometry allows
 * 16-byte accesses, the level-0 kernels read / write the pixels themselves -- Gray, Gray16, RGBA,
 * RGBA64, NRGBA, NRGBA64 alike (a fourth component is its own plane: encoder.go:152-179), and so do the
 * 9-7 level-0 kernels for image.RGBA and image.Gray on a lossy 8-bit plan (the reference's DefaultOptions); otherwise
 * the pixels pass through an int32 staging frame.  Same results either way.  On a shard (tile_first /
 * tile_count) the inverse writes the pixels of the shard's tiles only, either way. */
int j2k_plan_forward_pixels(j2k_plan *plan, int format, const void *d_pix, size_t stride, int32_t *d_coeff);
int j2k_plan_inverse_pixels(j2k_plan *plan, const int32_t *d_coeff, void *d_pix, size_t stride);
/* 1 when that call (inverse != 0: j2k_plan_inverse_pixels, format ignored) would take the fused
 * kernels for these pixels, 0 when it would stage; < 0 on bad arguments.  Launches nothing. */
int j2k_plan_pixels_fused(const j2k_plan *plan, int format, const void *d_pix, size_t stride, int inverse);
/* The 16-bit hand-off of level 1's input between the packed-RGBA8 level-0 launch and the one-launch deeper levels (context
 * option l0_scr16: bit 0 forward, bit 1 inverse; same results either way).  Bits: 1 = the plan allows it in
 * j2k_plan_forward_rgba8 / _forward_pixels(J2K_PIX_RGBA8) of a fused frame, 2 = in j2k_plan_inverse_rgba8 / _inverse_pixels
 * (rows that fit are stored 16-bit, chosen per row in every call), 4 / 8 = the plan's last forward / inverse call launched
 * the 16-bit kernels.  Launches nothing. */
int j2k_plan_scr16(const j2k_plan *plan);
/* Which forms of the MQ block coder the plan's last block encode and block decode took -- the library picks between a latency and a
 * throughput setting by the number of live contexts of this process that have built an MQ-coder plan (two or more: throughput), and
 * these calls say what that came to.  They launch nothing and change no launch.
 *   out[0]  contexts of this process that have built an MQ-coder plan and are still alive (a context counts once), now
 *   out[1]  blocks per wavefront (K) of the MQ chains of the last block encode; 0 = the one-kernel form ran (or no encode yet)
 *   out[2]  1 = that encode coded its blocks above 64 x 64 as two kernels through symbol lists
 *   out[3]  1 = the last block decode took the plane-stepped path, out[4] = its form (context option t1_dec_lanes; 0 otherwise)
 *   out[5]  launches of the decoder for blocks above 64 x 64 in that decode: 0 (no such block / another kernel took them), 1 or 2
 *   out[6]  1 = that decode wanted the plane-stepped path and fell back to the one-launch kernels (a stream that is not 16-byte
 *           aligned, or no room for the path's workspace)
 *   out[7]  reserved, 0
 * j2k_ctx_mq_forms: the same record of the context's last j2k_decode_blocks / _coarse / _floors (the host calls have no plan);
 * out[1] and out[2] are 0. */
int j2k_plan_mq_forms(const j2k_plan *plan, int32_t out[8]);
int j2k_ctx_mq_forms(const j2k_ctx *ctx, int32_t out[8]);

/* ---- the default branch of extractImageData (encoder.go:178-195) for the types Go's decoders return ----------------
 * Any other image.Image becomes 3 components at precision 8: r>>8, g>>8, b>>8 of img.At(x, y).RGBA(), then the
 * Options.Precision rescale as for every type.  So an image described here encodes exactly like the packed RGBA8 frame
 * (J2K_PIX_RGBA8, alpha ignored) of its converted colours, and every call below is that frame's call on the converted
 * colours.  Colours as Go's image/color (Go >= 1.8), for pixel (x, y) of Rect = [min_x, min_x + width) x [min_y, min_y + height)
 * and Go's truncating `/`:
 *   J2K_IMG_YCBCR     plane[0] = Y (yi = (y - min_y) * stride[0] + x - min_x), plane[1] = Cb, plane[2] = Cr at
 *                     ci = (y / vd - min_y / vd) * stride[k] + x / hd - min_x / hd, (hd, vd) by ratio: 444 (1, 1), 422 (2, 1),
 *                     420 (2, 2), 440 (1, 2), 411 (4, 1), 410 (4, 2).  color.YCbCr.RGBA(): v = Y * 0x10100 + (91881 Cr',
 *                     -22554 Cb' - 46802 Cr', 116130 Cb') with Cb' = Cb - 128, Cr' = Cr - 128; the sample = clamp(v, 0, 0xFFFFFF) >> 16.
 *   J2K_IMG_CMYK      plane[0] = Pix, 4 bytes C, M, Y, K per pixel: w = 0xFFFF - K * 0x101, r = (0xFFFF - C * 0x101) * w / 0xFFFF
 *                     (uint32; g, b from M, Y), the sample = r >> 8.
 *   J2K_IMG_PALETTED  plane[0] = Pix, 1 byte per pixel, indexing palette: npal <= 256 entries of Palette[i].RGBA() >> 8 as
 *                     3 bytes R, G, B (built by the caller).
 * Go panics -- J2K_ERR_GO_PANIC, nothing written -- when a plane is shorter (len) than the largest offset the rectangle
 * reaches, when npal == 0 (At returns nil) and when an index >= npal; the last is found on the device. */
enum { J2K_IMG_YCBCR = 16, J2K_IMG_CMYK = 17, J2K_IMG_PALETTED = 18 };
enum { J2K_YCBCR_444 = 0, J2K_YCBCR_422 = 1, J2K_YCBCR_420 = 2, J2K_YCBCR_440 = 3, J2K_YCBCR_411 = 4, J2K_YCBCR_410 = 5 };
typedef struct j2k_image {
    int32_t kind, ratio;                 /* J2K_IMG_*, J2K_YCBCR_* (YCbCr only) */
    int32_t min_x, min_y, width, height; /* Rect */
    const uint8_t *plane[3];             /* YCbCr: Y, Cb, Cr; CMYK / Paletted: Pix (plane[0] only) */
    int64_t stride[3];                   /* bytes per row of each plane (YCbCr: YStride, CStride, CStride) */
    uint64_t len[3];                     /* len() of each Go slice */
    const uint8_t *palette;              /* Paletted: npal x 3 bytes */
    int32_t npal, pad_;
} j2k_image;
/* Host only, no device: J2K_ERR_INVALID_ARG for an unknown kind / ratio, a negative size, a stride shorter than a row or
 * (width >= 0, height >= 0) dims other than these; J2K_ERR_GO_PANIC for a short plane or npal == 0 (as above). */
int j2k_image_validate(const j2k_image *img, int width, int height);
/* An image whose planes and palette are DEVICE memory (the descriptor itself is host memory, as in every call below that takes
 * d_img) -> packed RGBA8 frame (alpha 255, `stride` bytes per row, 4-byte aligned) on the ctx stream.  Paletted images synchronise
 * (the index check) and return J2K_ERR_GO_PANIC for an index >= npal. */
int j2k_image_to_rgba8(j2k_ctx *ctx, const j2k_image *d_img, void *d_pix, size_t stride);
/* HOST image -> ncomp = 3 planes of width x height int32 (caller-allocated), the mirror of j2k_extract_image_data; the planes
 * cross PCIe at their native sizes.  target_precision as there (0: 8 bit). */
int j2k_extract_image_planar(j2k_ctx *ctx, const j2k_image *img, int target_precision, int32_t *const *planes);
/* j2k_plan_forward_pixels(J2K_PIX_RGBA8) of the converted colours, DEVICE image.  YCbCr 4:4:4 / 4:2:2 / 4:2:0 images are read by
 * the 5-3 level-0 workgroup kernel itself when j2k_plan_image_fused says so; everything else converts into a staging RGBA8
 * frame first.  Paletted images synchronise (the index check) and return J2K_ERR_GO_PANIC without touching d_coeff. */
int j2k_plan_forward_image(j2k_plan *plan, const j2k_image *d_img, int32_t *d_coeff);
/* 1 when j2k_plan_forward_image would take the fused kernel for this image, 0 when it would stage; < 0 on bad arguments */
int j2k_plan_image_fused(const j2k_plan *plan, const j2k_image *d_img);
/* j2k_plan_encode_frame_pixels(J2K_PIX_RGBA8) of the converted colours (closed-loop plans, asynchronous); a paletted index
 * >= npal is J2K_ERR_GO_PANIC from the next j2k_plan_frame_status, and the tile-parts are then not the image's. */
int j2k_plan_encode_frame_image(j2k_plan *plan, const j2k_image *d_img, int sop, int eph, uint8_t *d_out, size_t cap,
                                uint64_t *d_tile_offs);
/* j2k_encode_pixels_host(J2K_PIX_RGBA8) of the converted colours for a HOST image: the planes cross PCIe at their native
 * sizes (the bytes the rectangle reaches); outputs as there.  J2K_ERR_GO_PANIC as above with nothing written. */
int j2k_encode_image_host(j2k_plan *plan, const j2k_image *img, int sop, int eph, uint8_t *out, size_t cap, size_t *out_len,
                          uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps);

/* ---- decode-side colour conversions to sRGB ---------------------------------
 * getColorConversion(cs)(componentData, precision) (colorspace.go:54-480); the values are the
 * reference's ColorSpace constants (jpeg2000.go:124-197).  Spaces without a conversion (sRGB, gray,
 * bilevel, unknown, unspecified) and component counts below what a conversion needs (3; 4 for
 * CMYK / YCCK) leave the data untouched, as the reference does. */
enum {
    J2K_CS_UNKNOWN = -1, J2K_CS_UNSPECIFIED = 0, J2K_CS_SRGB = 1, J2K_CS_GRAY = 2, J2K_CS_SYCC = 3, J2K_CS_EYCC = 4,
    J2K_CS_CMYK = 5, J2K_CS_BILEVEL = 6, J2K_CS_YCBCR2 = 7, J2K_CS_YCBCR3 = 8, J2K_CS_PHOTOYCC = 9, J2K_CS_CMY = 10,
    J2K_CS_YCCK = 11, J2K_CS_CIELAB = 12, J2K_CS_CIEJAB = 13, J2K_CS_ESRGB = 14, J2K_CS_ROMMRGB = 15,
    J2K_CS_YPBPR60 = 16, J2K_CS_YPBPR50 = 17
};
/* host planes (ncomp pointers to n int32 each), converted in place */
int j2k_convert_colorspace(j2k_ctx *ctx, int colorspace, int32_t *const *planes, int ncomp, size_t n, int precision);
/* device planes, contiguous (ncomp x n int32), converted in place on the ctx stream */
int j2k_convert_colorspace_device(j2k_ctx *ctx, int colorspace, int32_t *d_planes, int ncomp, size_t n, int precision);

/* Whole shard from HOST planes, mirroring encoder.preprocess + encodeTile
 * (encoder.go:216-281, 597-688): planes[c] = host int32 W*H, mutated in place to
 * the coefficients like e.componentData when the frame is a single tile (with tiles
 * the coefficients are returned tile-plane by tile-plane in `coeff` if non-NULL).
 * out receives the concatenated block bytes of all tiles in job order;
 * tile_offs[t] (tiles+1 entries) delimits each tile's data for SOT assembly. */
int j2k_encode_frame(j2k_plan *plan, int32_t *const *planes, int32_t *coeff, uint8_t *out, size_t cap,
                     size_t *out_len, uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps);

/* Pixels at native width from / to HOST memory, one synchronous call each: what a cgo jpeg2000.Encode / Decode binds when the image
 * lives in Go memory (encoder.go:79-213 + 216-281 + 597-688 + 746-760; decoder.go:363-588).  j2k_encode_pixels_host: pix (a Go Pix
 * layout, `stride` bytes per row) crosses PCIe at native width, out receives every tile of the shard as a tile-part -- reference-mode
 * plan: SOT | SOD | the tile's concatenated block bytes (createTileHeader of encodeTile's output); closed-loop plan: SOT | SOD | packets
 * (sop / eph used there only) -- *out_len the bytes (J2K_ERR_CAPACITY with *out_len set when cap is smaller), tile_offs[t] (tiles + 1, may
 * be NULL) where tile-part t starts, lens / numbps per code-block (may be NULL).  j2k_decode_pixels_host (closed-loop plans): the
 * tile-parts back to pixels of the plan's format (1 / 3 / 4 components, precision <= 8: Gray / RGBA, else Gray16 / RGBA64). */
int j2k_encode_pixels_host(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, uint8_t *out, size_t cap,
                           size_t *out_len, uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps);
int j2k_decode_pixels_host(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, void *pix, size_t stride);

/* ---- the pipelined host codec: the two calls above with up to `depth` frames in flight ---------------------------------------------------
 * A submitted encode IS j2k_encode_pixels_host on the same arguments (reference-mode and closed-loop plans, either coder), a submitted decode
 * IS j2k_decode_pixels_host (closed-loop plans; J2K_ERR_UNSUPPORTED from the submit otherwise): out, *out_len, tile_offs, lens, numbps and
 * pix are written byte for byte as those calls write them, but one frame's H2D and D2H copies run beside another frame's kernels.  Only the
 * plain forms: no budgets, layers, quality targets, roi, reduce, skip_planes, truncated streams, area or image sources.
 *   How.  All kernels of all frames run on the context's one stream in submission order; each of the `depth` slots owns the device pixels,
 * the device tile-parts with their offsets, and a snapshot of the frame's status (taken, and the plan's status word cleared, on the stream
 * behind the frame's kernels: a refused frame never disturbs its neighbours).  The pipe owns one high-priority stream per copy direction.
 * The small results come back first; a frame's tile-parts are copied at their exact length once that length is on the host, which happens
 * inside a later submit, poll or wait -- the library creates no thread, reads no environment variable, and a steady-state submit allocates
 * nothing (everything is allocated by j2k_pipe_create, or at the first frame that needs the ring for pageable memory or a larger stride).
 *   Caller memory.  The pipe asks hipPointerGetAttributes whether pix, out and cs are pinned (j2k_host_alloc, hipHostMalloc,
 * hipHostRegister).  Pinned input is copied from where it lies; pinned tile-part output receives the D2H copy; a pinned decode frame is
 * stored by the inverse transform itself through its device address (no device frame, no copy) unless that address is not aligned to what
 * the device call takes (4 bytes for RGBA rows, the sample size for gray), in which case it takes the slot's device frame and a copy.
 * Pageable memory (Go's heap) is staged through a pinned ring owned by the pipe: memcpy in inside the submit, memcpy out inside the wait.
 * Results are identical in every case; row padding of a decoded frame is never written.  Buffers handed to a submit stay valid and
 * untouched by the caller until that ticket's wait returns.
 *   Tickets are 1, 2, 3, ... per pipe; frames complete in submission order; waits may come in any order.  At most `depth` tickets may be
 * un-waited: a further submit returns J2K_ERR_INVALID_ARG, queues nothing and consumes no ticket -- as does every refusal the one-call form
 * decides from its arguments and the plan (NULL pointers, format / stride, a decode on a plan without closed_loop, a capturing context), with
 * that form's code.  j2k_pipe_wait returns what the one-call form would have returned for that frame: J2K_OK; J2K_ERR_CAPACITY with *out_len
 * = what the tile-parts take and out untouched; J2K_ERR_INVALID_ARG for a malformed stream, pix untouched in every memory case;
 * J2K_ERR_HIP.  *out_len (may be NULL) is set for encodes.  A ticket that is unknown or was waited before: J2K_ERR_INVALID_ARG.
 * j2k_pipe_poll never blocks: *done = 1 once the wait would not block.  j2k_pipe_drain returns when all submitted work is complete; the
 * tickets stay waitable.  j2k_pipe_destroy drains, frees everything and leaves the plan usable by the one-call forms.
 *   While tickets are outstanding the plan and its context belong to the pipe: no other call on either (the library does not police it).
 * The pipe must be destroyed before its plan.  Single-threaded, like the context.
 *   j2k_host_alloc / j2k_host_free: pinned host memory (hipHostMalloc), so that a cgo caller needs no HIP binding; NULL on failure. */
typedef struct j2k_pipe j2k_pipe;
int j2k_pipe_create(j2k_plan *plan, int depth, j2k_pipe **out);       /* depth 1 ... 8 frames in flight */
void j2k_pipe_destroy(j2k_pipe *pipe);
int j2k_pipe_submit_encode(j2k_pipe *pipe, int format, const void *pix, size_t stride, int sop, int eph, uint8_t *out, size_t cap,
                           uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps, uint64_t *ticket);
int j2k_pipe_submit_decode(j2k_pipe *pipe, const uint8_t *cs, size_t len, int sop, int eph, void *pix, size_t stride, uint64_t *ticket);
int j2k_pipe_wait(j2k_pipe *pipe, uint64_t ticket, size_t *out_len);
int j2k_pipe_poll(j2k_pipe *pipe, uint64_t ticket, int *done);
int j2k_pipe_drain(j2k_pipe *pipe);
void *j2k_host_alloc(size_t bytes);
void j2k_host_free(void *p);

/* ---- multi-tile codestream assembly: host calls, no device needed ------------------------------
 * j2k_create_tile_header = encoder.createTileHeader(tileIdx, tileData) (encoder.go:746-760): SOT (0xFF90) Lsot = 10,
 * Isot = uint16(tileIdx), Psot = uint32(14 + len), TPsot = 0, TNsot = 1, SOD (0xFF93), then the tile data -- 14 + len bytes.
 * j2k_assemble_tiles applies it to every tile of a (gathered) stream, tile t = stream[tile_offs[t], tile_offs[t+1]) with
 * index tile_first + t, tile-parts laid end to end: what rank 0 hands to the Go side between the main header and EOC
 * (the reference's generateTiles, encoder.go:568-579, emits tile 0 only). */
size_t j2k_tile_part_bound(const uint64_t *tile_offs, int ntiles);
int j2k_create_tile_header(int tile_idx, const uint8_t *tile_data, size_t len, uint8_t *out, size_t cap, size_t *out_len);
int j2k_assemble_tiles(const uint8_t *stream, const uint64_t *tile_offs, int tile_first, int ntiles, uint8_t *out, size_t cap,
                       size_t *out_len);
/* The same on device buffers, for a plan's shard: every tile of d_stream / d_offs (as j2k_plan_encode_stream or
 * j2k_plan_unpack_stream made them) becomes a tile-part with index tile_first + t, laid end to end in d_out
 * (j2k_plan_tile_parts_bound bytes at most); *d_out_len (device) = the bytes written.  Asynchronous on the context's
 * stream: one D2H copy then carries finished tile-parts instead of a stream the host still has to cut up. */
size_t j2k_plan_tile_parts_bound(const j2k_plan *plan);
int j2k_plan_assemble_tiles_device(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, uint8_t *d_out, uint64_t *d_out_len);
/* codestream.Parser.ReadTilePartHeader (internal/codestream/parser.go:894-983): the SOT fields of the tile-part whose SOT
 * marker is at cs[pos], its in-header marker segments skipped by length (parser.go:180-190; their contents stay with the
 * Go-side parser: header_off / header_markers say where they are), and where its data lies (Psot = 0: to the end).
 * Errors as the parser's: Lsot != 10, a segment length < 2, truncated input -> J2K_ERR_INVALID_ARG. */
typedef struct j2k_tile_part {
    uint16_t tile_index;          /* Isot  */
    uint8_t tile_part_index;      /* TPsot */
    uint8_t num_tile_parts;       /* TNsot */
    uint32_t tile_part_length;    /* Psot  */
    uint32_t header_markers;      /* marker segments between the SOT segment and SOD */
    uint32_t pad_;
    uint64_t header_off;          /* offset of the first of them (== data_off - 2 when there are none) */
    uint64_t data_off, data_len;  /* the tile-part's data */
} j2k_tile_part;
int j2k_read_tile_part_header(const uint8_t *cs, size_t len, size_t pos, j2k_tile_part *tp);
/* every tile-part of a run of tile-parts (up to EOC or the end); *nparts = how many there are (J2K_ERR_CAPACITY if > cap) */
int j2k_parse_tile_parts(const uint8_t *cs, size_t len, j2k_tile_part *parts, size_t cap, size_t *nparts);

/* ---- Tier-2 packet coding and tile geometry: host calls, no device needed -------------------------
 * The reference's internal/tcd/t2.go and the geometry of tcd.go, reproduced as they are written -- the "tag tree" values
 * are unary (t2.go:368-377), the length-of-length field is 3 bits and wraps for blocks of 128 bytes or more
 * (t2.go:408-437), PCRL runs every component / resolution to the LARGEST precinct count (t2.go:86-114), the packet
 * decoder's Position() moves over markers and bodies only (t2.go:463-503) -- because parity with the reference is the
 * contract; none of this is a conformant Part-1 packet stream (SURVEY 8f calls a conformant mode "explicitly outside
 * reference parity").  In the reference only tests call t2.go; decoder.go:312,373 calls the geometry.
 *
 * j2k_t2_packet_sequence = NewPacketIterator + Next() until exhausted (t2.go:41-238), progression order
 * 0..4 = LRCP, RLCP, RPCL, PCRL, CPRL (codestream/markers.go:177-188; any other order yields no packet, t2.go:86-100).
 * precincts [][][]int is passed flat: prec_ncomp = len(precincts), prec_nres[c] = len(precincts[c]),
 * prec_counts = precincts[c][r][0] for c, r in order (a (c, r) the table does not cover counts as one precinct).
 * *count = packets in the sequence; J2K_ERR_CAPACITY (with *count set) when cap is smaller. */
typedef struct j2k_packet { int32_t layer, resolution, component, precinct; } j2k_packet;
int j2k_t2_packet_sequence(int ncomp, int nres, int nlayers, const int32_t *prec_counts, const int32_t *prec_nres, int prec_ncomp,
                           int order, j2k_packet *out, size_t cap, size_t *count);

/* A precinct as the packet coder sees it (tcd.go:86-128): nbands lists of code-blocks (band_ncb[b] each, flat in cbs) and
 * the widths of its two tag trees (only used as divisors: a width of 0 is the Go divide panic, J2K_ERR_GO_PANIC).
 * Code-block fields: IncludedInLayers, ZeroBitPlanes, len(Passes), Data (data_len bytes at data; data_cap = room the
 * decoder may fill). */
typedef struct j2k_t2_cb {
    int32_t included_in_layers, zero_bit_planes, num_passes;
    uint32_t data_len, data_cap, pad_;
    uint8_t *data;
} j2k_t2_cb;
typedef struct j2k_t2_precinct {
    int32_t nbands, incl_tree_w, imsb_tree_w, pad_;
    const int32_t *band_ncb;
    j2k_t2_cb *cbs;
} j2k_t2_precinct;
/* PacketEncoder.EncodePacket (t2.go:250-290): [SOP FF91 0004 uint16(layer)] header bits through the byte-stuffing
 * writer (bio.go:157-226: after a 0xFF byte the next byte holds 7 bits), flushed; [EPH FF92]; the bodies of the
 * code-blocks with IncludedInLayers <= layer and data.  *bio_delay carries the writer's "last byte was 0xFF" flag from
 * one packet of an encoder to the next (0 for a new encoder).  j2k_t2_packet_bound: an upper bound of *len. */
size_t j2k_t2_packet_bound(const j2k_t2_precinct *p);
int j2k_t2_encode_packet(const j2k_t2_precinct *p, int layer, int sop, int eph, uint8_t *bio_delay, uint8_t *out, size_t cap, size_t *len);
/* PacketDecoder.DecodePacket (t2.go:463-503) on data[0, len): the decoder object's state is the caller's -- pos
 * (Position(): markers and bodies), and the header bit reader's own position / byte / bit count / "saw 0xFF"
 * (a zeroed struct is NewPacketDecoder).  Fills the code-blocks' fields; a block's data is zeroed to its decoded length
 * (J2K_ERR_CAPACITY if data_cap is smaller) and then filled from the body.  Running out of header bits or body bytes is
 * the reference's error return: J2K_ERR_INVALID_ARG. */
typedef struct j2k_t2_dec_state { uint64_t pos, rpos; uint8_t buf, cnt, saw_ff, pad_[5]; } j2k_t2_dec_state;
int j2k_t2_decode_packet(const uint8_t *data, size_t len, j2k_t2_dec_state *st, j2k_t2_precinct *p, int layer, int sop, int eph);
/* PacketEncoder.EncodePacket for a RUN of packets on DEVICE buffers (csrc/t2dev.hip): packet i is coded by the same encoder
 * right after packet i - 1, so the writer's "last byte was 0xFF" flag runs through the run (*bio_delay in and out, as above).
 * A packet = its layer, the widths of its two tag trees (divisors only) and ncb code-blocks from d_cbs[cb0] (a table of ncbs) in coding order
 * (band after band: the band structure changes nothing in the bytes, t2.go:320-364); a code-block's bytes are data_len bytes
 * at d_data + data_off (e.g. the compacted stream of j2k_plan_encode_stream).  Packet i lands at d_out + d_offs[i]
 * (d_offs: npackets + 1 entries, the last = *total).  J2K_ERR_CAPACITY (with *total set, nothing written) when cap is
 * smaller; J2K_ERR_GO_PANIC for a tree width of 0 that the coder divides by.  Synchronises the context's stream. */
typedef struct j2k_t2_dev_cb { int32_t included_in_layers, zero_bit_planes, num_passes; uint32_t data_len; uint64_t data_off; } j2k_t2_dev_cb;
/* flags: 0 = the reference's coder.  The closed-loop mode (j2k_params.closed_loop; NOT the reference) sets
 *   J2K_T2_FRESH     this packet is the first of a new PacketEncoder / PacketDecoder object (one per tile): the byte-stuffing
 *                    writer's / reader's "last byte was 0xFF" flag starts clear
 *   J2K_T2_WIDE_LEN  the length-of-length field has 5 bits (the reference's 3 wrap for blocks of 128 bytes or more, t2.go:408-437)
 *   J2K_T2_SEATED    decoder only: the header is read from Position() and Position() moves past it (the reference's header
 *                    reader runs over the buffer on its own and Position() only moves over markers and bodies, t2.go:463-503)
 *   J2K_T2_LAYERED   decoder, the j2k_plan_*_layers calls only (every other call ignores it): the packet belongs to a layered stream -- the header
 *                    of layer l > 0 carries one "contributes" bit per block, ZeroBitPlanes behind it iff the block has not contributed before,
 *                    then the passes and the length of the layer's INCREMENT ("Quality layers" below) */
#define J2K_T2_FRESH 1
#define J2K_T2_WIDE_LEN 2
#define J2K_T2_SEATED 4
#define J2K_T2_LAYERED 8
typedef struct j2k_t2_dev_packet { int32_t layer, incl_tree_w, imsb_tree_w, flags; int64_t cb0, ncb; } j2k_t2_dev_packet;
int j2k_t2_encode_packets_device(j2k_ctx *ctx, const j2k_t2_dev_packet *d_packets, size_t npackets, const j2k_t2_dev_cb *d_cbs, size_t ncbs,
                                 const uint8_t *d_data, int sop, int eph, uint8_t *bio_delay, uint8_t *d_out, size_t cap,
                                 uint64_t *d_offs, size_t *total);
/* PacketDecoder.DecodePacket (t2.go:463-652) for a RUN of packets by ONE decoder object on a DEVICE buffer d_data[0, len)
 * (csrc/t2dec.hip): packet i is decoded right after packet i - 1 with the object's state -- *st in and out, as
 * j2k_t2_decode_packet's (a zeroed struct is NewPacketDecoder).  d_cbs is read AND written (IncludedInLayers persists from
 * layer to layer): a block the packet includes gets IncludedInLayers, ZeroBitPlanes, len(Passes), len(Data) = data_len and
 * data_off = where its body lies in d_data (nothing is copied).  *packets_done = packets decoded before the first error;
 * the status is that packet's: J2K_ERR_INVALID_ARG for the reference's error returns (out of header bits, a body past the
 * end), J2K_ERR_GO_PANIC for a tree of width 0 it divides by.  Synchronises the context's stream. */
int j2k_t2_decode_packets_device(j2k_ctx *ctx, const j2k_t2_dev_packet *d_packets, size_t npackets, j2k_t2_dev_cb *d_cbs, size_t ncbs,
                                 const uint8_t *d_data, size_t len, int sop, int eph, j2k_t2_dec_state *st, size_t *packets_done);

/* ---- the closed-loop frame codec (j2k_params.closed_loop = 1): tile-parts of packets out, pixels back -------
 * The reference has the pieces -- PacketEncoder / PacketDecoder (t2.go), createTileHeader (encoder.go:746-760),
 * DecodeCodeBlock and ApplyInverseDWT (tcd.go:393-437) -- but no decode body (decoder.decodeTile is a placeholder,
 * decoder.go:375-411).  These calls are that body on device buffers, asynchronous on the context's stream:
 *   j2k_plan_encode_tile_parts  the block coder's outputs (j2k_plan_encode_stream) -> for every tile of the shard
 *                               SOT | SOD | one packet per (component, resolution) in job order, tile-parts end to end in
 *                               d_out (j2k_plan_frame_bound bytes at most); d_tile_offs[t] (tiles + 1, device) = where
 *                               tile-part t starts, the last entry the total.  Code-block fields as j2k_plan_t2_fill_cbs
 *                               with mb = 31, an empty block IncludedInLayers 1; a new PacketEncoder per tile.
 *                               cap < the bytes needed: nothing is written and d_tile_offs[tiles] holds the need
 *                               (J2K_ERR_CAPACITY from the next j2k_plan_frame_status).
 *   j2k_plan_decode_tile_parts  the inverse: d_cs[0, len) -> d_offs / d_lens / d_numbps as j2k_plan_decode_blocks takes
 *                               them (a block's bytes stay where they are in d_cs: d_offs points into it).  d_tile_offs
 *                               (device, tiles + 1) where the caller knows the tile-parts' positions (the Go-side parser
 *                               has read the SOT segments, parser.go:894-983; or the encode call's own table), else NULL:
 *                               the call walks the SOT segments itself (Psot), one after the other.
 *                               With sop != 0 and eph != 0 a tile's packets are parsed side by side: their starts are guessed from
 *                               the FF91 / FF92 markers, every packet is decoded on its own, and the result is kept only if each
 *                               packet ended in exactly the state the next one was started from -- otherwise (a marker pair inside
 *                               a body, a damaged header) that tile is decoded again one packet after the other.  The output is
 *                               the serial decoder's either way (j2k_ctx_set_option "t2_parallel" = 0: serial only).
 *   j2k_plan_frame_parallel_tiles  diagnostic: synchronises; *tiles = tiles whose packets were parsed side by side in the
 *                               decode calls since the last query
 *   j2k_plan_place_blocks       decoded blocks (j2k_plan_decode_blocks) -> each at its window of the coefficient planes
 *   j2k_plan_frame_status       synchronises and reports what the asynchronous calls above found since the last call:
 *                               J2K_OK, J2K_ERR_CAPACITY, or J2K_ERR_INVALID_ARG for a malformed tile-part / packet
 *   j2k_plan_encode_frame_pixels / j2k_plan_decode_frame_pixels   the whole chain with the plan's own workspaces:
 *                               pixels (any format, as j2k_plan_forward_pixels) -> tile-parts, and tile-parts -> pixels.  Same bytes
 *                               and pixels as the stage calls, with less copying: the encoder gathers every block once from its
 *                               coding slot into its packet in its tile-part (no dense stream in between); on an HT plan the
 *                               block decoder writes only the rows the reference's HT decoder writes (one in four), straight
 *                               into each block's window of coefficient planes the plan zeroed once.
 *                               j2k_plan_decode_frame_pixels writes nothing into d_pix while the plan's status word is set -- by a
 *                               tile-part or packet this call refused, or by an earlier call whose status was never read.
 * All of them return J2K_ERR_UNSUPPORTED on a plan without closed_loop. */
size_t j2k_plan_frame_bound(const j2k_plan *plan);
int j2k_plan_encode_tile_parts(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                               int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs);
int j2k_plan_decode_tile_parts(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                               uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps);
int j2k_plan_place_blocks(j2k_plan *plan, const int32_t *d_decoded, int32_t *d_coeff);
int j2k_plan_frame_status(j2k_plan *plan);
int j2k_plan_frame_parallel_tiles(j2k_plan *plan, long *tiles);
int j2k_plan_encode_frame_pixels(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                 uint8_t *d_out, size_t cap, uint64_t *d_tile_offs);
int j2k_plan_decode_frame_pixels(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                 void *d_pix, size_t stride);

/* ---- reduced-resolution decode of a Mallat plan (j2k_params.closed_loop = J2K_CLOSED_LOOP_MALLAT): Config.ReduceResolution -------
 * reduce = r runs the inverse levels L-1 ... r only (L = num_resolutions - 1) and takes LL_r as the frame: inverse RCT / ICT, DC shift
 * and the pixel pack at ceil(W / 2^r) x ceil(H / 2^r), the reference's output size (decodeTiles, decoder.go:289-295: (w + 1) / 2 per
 * step; the reference itself decodes no pixels there).  Tile (x0, y0, w, h) lands at (x0 >> r, y0 >> r) with ceil(w / 2^r) x
 * ceil(h / 2^r) samples.  Explicit calls, not plan state: a captured graph means what it says.
 *   J2K_ERR_UNSUPPORTED   a plan that is not Mallat
 *   J2K_ERR_INVALID_ARG   reduce < 0 or > L; a tiled frame whose tile_w or tile_h is not a multiple of 2^r; a batch whose frame_rows
 *                         is not a multiple of 2^r (the reduced tiles would not cover the reduced frame exactly once)
 * reduce = 0 is exactly the call without it.  d_frame = [C][H_r][W_r] int32; pixels in the plan's own format, as
 * j2k_plan_inverse_pixels; a shard writes its own tiles only.  The decode calls parse every packet (a tile's packets are in component ->
 * resolution order) but decode and place only the code-blocks of the resolutions <= num_resolutions - 1 - r -- with the MQ coder the
 * block decoder is where the time is -- and, like j2k_plan_decode_frame_pixels, write nothing into d_pix while the plan's status word
 * is set.  The tables of an r are made at its first use (so: once before j2k_ctx_capture_begin) and kept in the plan. */
int j2k_plan_reduced_size(const j2k_plan *plan, int reduce, int32_t *width, int32_t *height);
int j2k_plan_inverse_reduced(j2k_plan *plan, const int32_t *d_coeff, int reduce, int32_t *d_frame);
int j2k_plan_inverse_pixels_reduced(j2k_plan *plan, const int32_t *d_coeff, int reduce, void *d_pix, size_t stride);
int j2k_plan_decode_frame_pixels_reduced(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs,
                                         int sop, int eph, int reduce, void *d_pix, size_t stride);
int j2k_decode_pixels_host_reduced(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int reduce,
                                   void *pix, size_t stride);
/* Both scalability axes in one call: `reduce` as above (0 on any closed-loop plan, > 0 by the rules of the _reduced calls) and the
 * quality floor `skip_planes` of j2k_decode_blocks_coarse (uniform over the frame: there are no quality layers in the stream).  An
 * argument, not plan state, like `reduce`: a captured graph means what it says.  skip_planes = 0 is the _reduced call (reduce = 0:
 * j2k_plan_decode_frame_pixels).  A refused call writes nothing into d_pix / pix. */
int j2k_plan_decode_blocks_coarse(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                  const uint8_t *d_numbps, int skip_planes, int32_t *d_decoded);
int j2k_plan_decode_frame_pixels_coarse(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs,
                                        int sop, int eph, int reduce, int skip_planes, void *d_pix, size_t stride);
int j2k_decode_pixels_host_coarse(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int reduce,
                                  int skip_planes, void *pix, size_t stride);
/* A floor per block beside the uniform one (MQ coder): block j's decoder stops after bit plane max(skip_planes, floors[j]) -- by the same
 * loop bound or plane shift, in every decode kernel form -- and its result is that of the _coarse call at that floor.  floors: one byte
 * per block, 0 ... 31 (j2k_decode_blocks_floors: host memory, checked, J2K_ERR_INVALID_ARG; j2k_plan_decode_blocks_floors: device memory,
 * not checked -- a block whose floor is at or above its numBPS is zeros).  floors = NULL is the _coarse call; floors != NULL with
 * J2K_CODER_HT: J2K_ERR_UNSUPPORTED.  The calls without floors behave as before on every input. */
int j2k_decode_blocks_floors(j2k_ctx *ctx, int coder, const uint8_t *bytes, const uint64_t *offs, const uint32_t *lens,
                             const uint8_t *numbps, const j2k_block *blocks, size_t nblocks, int skip_planes,
                             const uint8_t *floors, int32_t *coeffs, const uint64_t *coeff_offs);
int j2k_plan_decode_blocks_floors(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                  const uint8_t *d_numbps, int skip_planes, const uint8_t *d_floors, int32_t *d_decoded);

/* ---- rate control of the MQ block coder (a feature of this library: the reference reads Options.CompressionRatio nowhere) ----------
 * "Which bit planes of which blocks fit N bytes best": the block encoder fills a rate table per block, a second kernel the matching
 * distortions, a third one allocates the budget.  Tables have 32 entries per job, entry p = "the first p bit planes kept", p = 0 ...
 * numBPS (numBPS <= 31); tests/rate_cases.py is the definition the device agrees with bit for bit.
 *   d_rate[j * 32 + p]   uint32: bytes of block j's codeword (a prefix of the bytes j2k_plan_encode_blocks writes, which are unchanged)
 *                        whose decode has the first p planes right: with k = numBPS - p, |decoded| >> k == |v| >> k and the signs
 *                        agree wherever that is not 0 (the decoder feeds 0xFF past the end of its data, mqc.go:402-413).  [0] = 0,
 *                        [numBPS] = d_lens[j], non-decreasing; the entries above numBPS repeat d_lens[j].  A bound, not the minimum:
 *                        the coder's byte index at the plane's end + 5, capped at the length (DESIGN.md 7 has the argument)
 *   d_dist[j * 32 + p]   uint64: sum over the block of (|v| - |coarse(v, k)|)^2, coarse = the result of j2k_decode_blocks_coarse at
 *                        floor k, wrapping arithmetic; [numBPS] = 0 and so are the entries above
 * j2k_plan_encode_blocks_planes   j2k_plan_encode_blocks + both tables (the same slots, lens and numbps)
 * j2k_plan_rate_allocate          d_kept[j] = planes kept of block j, *d_chosen = sum of d_rate[j * 32 + d_kept[j]] <= max_body_bytes.
 *                                 Nothing is cut if the full lengths fit.  Otherwise every block's choice is the last point of its convex
 *                                 hull of (rate, weight * distortion) whose slope is >= lambda, and lambda is the smallest float64 (by bit
 *                                 pattern, found by 64 steps of bisection) whose choices fit: one workgroup, integer sums, reproducible
 *                                 bit for bit.  The budget counts CODE-BLOCK BODY bytes; packet and tile-part headers come on top.
 * j2k_plan_get_rate_weights /     the weight of every (component, resolution, band): ncomp * num_resolutions * 4 float64, index
 * j2k_plan_set_rate_weights       (c * num_resolutions + r) * 4 + band.  Default on a Mallat plan: the synthesis energy gain of the band
 *                                 (the 1-D synthesis low-pass / high-pass impulse responses iterated through the levels), component
 *                                 weight 1; on other plans the windows are not sub-bands and every weight is 1 -- weights other than 1
 *                                 mean something in Mallat mode only.  set(NULL, 0) restores the default; weights are finite and >= 0.
 * J2K_ERR_UNSUPPORTED: an HT plan, a plan without closed_loop, a batch plan (frame_rows), a plan with blocks above 64 x 64.
 * J2K_ERR_INVALID_ARG: a negative budget.  Both before anything is launched.
 * j2k_plan_encode_tile_parts_kept    j2k_plan_encode_tile_parts with block j cut after its first d_kept[j] planes: its bytes are the prefix
 *                                    d_rate[j * 32 + d_kept[j]], its passes the 3 p - 2 of those planes (p = 0: no passes, no bytes, in no
 *                                    layer), ZeroBitPlanes = 31 - numBPS as before -- today's byte format.  d_kept[j] = numBPS everywhere
 *                                    gives j2k_plan_encode_tile_parts' bytes.
 * j2k_plan_decode_tile_parts_floors  j2k_plan_decode_tile_parts + each block's floor: d_floors[j] = max(31 - ZeroBitPlanes - (passes + 2) / 3,
 *                                    0), d_numbps[j] = (passes + 2) / 3 + d_floors[j]; j2k_plan_decode_blocks_floors decodes that.  The
 *                                    calls without floors keep their rule (numbps = (passes + 2) / 3) on every input.
 * j2k_plan_encode_frame_pixels_rate  j2k_plan_encode_frame_pixels with at most max_body_bytes of code-block bodies (headers on top: the
 *                                    last entry of d_tile_offs says what the frame took); a budget that cuts nothing gives its bytes.
 * j2k_plan_decode_frame_pixels_rate  j2k_plan_decode_frame_pixels_coarse for such streams: block j runs down to max(skip_planes, its floor);
 *                                    reduce as there.
 * j2k_encode_pixels_host_rate /      the synchronous host-memory forms (j2k_encode_pixels_host / j2k_decode_pixels_host_coarse); lens and
 * j2k_decode_pixels_host_rate        numbps of the encode are the UNCUT lengths and plane counts.
 * No budget that includes headers; pass-level truncation: the _passes calls further down; quality layers: the _layers calls below. */
int j2k_plan_encode_tile_parts_kept(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                    const uint8_t *d_numbps, const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph,
                                    uint8_t *d_out, size_t cap, uint64_t *d_tile_offs);
int j2k_plan_decode_tile_parts_floors(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                      uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors);
int j2k_plan_encode_frame_pixels_rate(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                      int64_t max_body_bytes, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs);
int j2k_plan_decode_frame_pixels_rate(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                      int reduce, int skip_planes, void *d_pix, size_t stride);
int j2k_encode_pixels_host_rate(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, int64_t max_body_bytes,
                                uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps);
int j2k_decode_pixels_host_rate(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int reduce, int skip_planes,
                                void *pix, size_t stride);
int j2k_plan_encode_blocks_planes(j2k_plan *plan, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps,
                                  uint32_t *d_rate, uint64_t *d_dist);
int j2k_plan_rate_allocate(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                           int64_t max_body_bytes, uint8_t *d_kept, uint64_t *d_chosen);
int j2k_plan_get_rate_weights(j2k_plan *plan, double *weights, size_t cap, size_t *count);
int j2k_plan_set_rate_weights(j2k_plan *plan, const double *weights, size_t count);

/* Quality layers (the library's own; the reference declares Options.NumLayers / Config.QualityLayers and only ever writes layer 0).  One encode
 * with L cumulative budgets of code-block body bytes, layer_bytes[0] <= ... <= layer_bytes[L - 1], 1 <= L <= J2K_MAX_LAYERS, yields ONE stream:
 * every tile-part is SOT | SOD | the tile's packet sequence once per layer, the layer outermost, so a byte prefix of every tile-part that ends at
 * a layer's end is a lower-quality version of the frame.  Layer l's cuts are those of j2k_plan_rate_allocate for layer_bytes[l]; a block's bytes
 * in layer l are its codeword between the cuts of layers l - 1 and l.  Format and reader rule: DESIGN.md 7; definition: tests/layer_cases.py.
 * L = 1 is byte for byte the stream of the _rate / _kept calls.  Plans: as j2k_plan_rate_allocate (closed-loop MQ, blocks <= 64 x 64, no batch),
 * else J2K_ERR_UNSUPPORTED; L outside 1 ... 32, a negative or a decreasing budget: J2K_ERR_INVALID_ARG.  The tables of a layer count are made at
 * its first use and kept in the plan (capture: run the call once before).
 *   j2k_plan_rate_allocate_layers      all L allocations in one launch: d_kept[l * blocks + j], d_chosen[l]; layer_bytes is host memory
 *   j2k_plan_encode_tile_parts_layers  the block coder's outputs + d_kept (L x blocks) + d_rate -> layered tile-parts; d_layer_offs[t * L + l] =
 *                                      where layer l of tile t ENDS in d_out (the last one = d_tile_offs[t + 1])
 *   j2k_plan_decode_tile_parts_layers  reads the first `layers` layers of every tile-part (whatever follows them up to the tile-part's end is
 *                                      ignored: the reader needs no L) and gathers every block's segments into d_dense (dense_cap bytes; the
 *                                      stream's length always suffices): d_offs / d_lens (into d_dense) / d_numbps / d_floors as the _floors
 *                                      calls give them -- j2k_plan_decode_blocks_floors decodes them from d_dense.  More layers than the stream
 *                                      holds: the packet decoder's error (J2K_ERR_INVALID_ARG in j2k_plan_frame_status)
 *   j2k_plan_frame_bound_layers        capacity that always suffices for an L-layer frame
 *   j2k_plan_encode_frame_pixels_layers / j2k_plan_decode_frame_pixels_layers   the frame calls (decode: layers, reduce and skip_planes together)
 *   j2k_encode_pixels_host_layers / j2k_decode_pixels_host_layers               the synchronous host-memory forms
 *   j2k_tile_parts_keep_layers         HOST ONLY, no device: the stream cut to its first `keep` layers (Psot patched), out_tile_offs[ntiles + 1]
 * No sub-plane truncation of a layered stream (the _passes calls cut single-layer streams), no header bytes in the budgets, no HT, no conformant Part-1 packet headers, no main header that carries L. */
#define J2K_MAX_LAYERS 32
int j2k_plan_rate_allocate_layers(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                                  const int64_t *layer_bytes, int nlayers, uint8_t *d_kept, uint64_t *d_chosen);
int j2k_plan_encode_tile_parts_layers(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                      const uint8_t *d_numbps, const uint8_t *d_kept, const uint32_t *d_rate, int nlayers, int sop, int eph,
                                      uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs);
int j2k_plan_decode_tile_parts_layers(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                      int layers, uint8_t *d_dense, size_t dense_cap, uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps,
                                      uint8_t *d_floors);
size_t j2k_plan_frame_bound_layers(const j2k_plan *plan, int nlayers);
int j2k_plan_encode_frame_pixels_layers(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                        const int64_t *layer_bytes, int nlayers, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                        uint64_t *d_layer_offs);
int j2k_plan_decode_frame_pixels_layers(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                        int layers, int reduce, int skip_planes, void *d_pix, size_t stride);
int j2k_encode_pixels_host_layers(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes,
                                  int nlayers, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs,
                                  uint32_t *lens, uint8_t *numbps);
int j2k_decode_pixels_host_layers(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int layers, int reduce,
                                  int skip_planes, void *pix, size_t stride);
int j2k_tile_parts_keep_layers(const uint8_t *cs, size_t len, const uint64_t *tile_offs, const uint64_t *layer_offs, int ntiles, int nlayers,
                               int keep, uint8_t *out, size_t cap, size_t *out_len, uint64_t *out_tile_offs);

/* Region decode (the library's own; the reference declares Config.DecodeArea and never reads it): the pixels of a rectangle of the frame,
 * decoding only the code-blocks that rectangle needs.  `area` is half-open, in full-resolution frame coordinates, 0 <= x0 < x1 <= W and
 * 0 <= y0 < y1 <= H.  With `reduce` = r the result is the rectangle [ceil(x0 / 2^r), ceil(x1 / 2^r)) x [ceil(y0 / 2^r), ceil(y1 / 2^r)) of
 * the reduced frame, bit for bit what the call without `area` writes there.
 *   The need set (definition: tests/area_cases.py).  Per tile the rectangle is cut to the tile and walked down the synthesis of
 * the wavelet: at level l an interval [a, b) of a dimension of n samples needs the low-pass samples [max(0, a / 2 - m), min(ceil(n / 2),
 * (b - 1) / 2 + m + 1)) and the high-pass samples [max(0, a / 2 - m), min(n / 2, (b - 1) / 2 + m + 1)), m = 1 for the 5-3 and 2 for the 9-7;
 * the low-pass interval goes on to level l + 1.  A code-block is needed iff its window meets one of these rectangles of the plane.  One
 * launch computes the set from the rectangle (a kernel argument: no host table per rectangle, no synchronisation) and empties the parsed
 * table entries of every other block, which the MQ block decoders turn into zeros without reading a byte of them.  Every packet is still
 * parsed and the inverse transform runs on the whole (reduced) frame into a staging frame of the plan; a rectangle pack writes the window to
 * d_pix at origin (0, 0), rows of `stride` bytes, under the frame status word (a refused stream leaves d_pix alone).
 *   Plans: Mallat, MQ coder, one frame, every tile (J2K_ERR_UNSUPPORTED for prefix-layout, HT, batch and shard plans).  A rectangle that is
 * inverted, empty, outside the frame or empty after `reduce`, or a stride shorter than a row of the result: J2K_ERR_INVALID_ARG.  What the
 * call without `area` refuses (reduce, skip_planes, layers) is refused in the same way.  Every refusal comes before the first launch.
 *   j2k_plan_area_shape               HOST ONLY: width and height of the result
 *   j2k_plan_area_blocks              the need set alone: d_need[j] = 1 iff job j is needed (device, one byte per job; asynchronous)
 *   j2k_plan_decode_frame_pixels_area the frame call with every axis: layers (0: not a layered stream, else the first `layers` layers as
 *                                     j2k_plan_decode_frame_pixels_layers), truncated (non-zero: per-block floors as the _rate call), reduce,
 *                                     skip_planes
 *   j2k_decode_pixels_host_area       its synchronous host-memory form; pix is written only if the stream was accepted
 * The tables of the need-set launch are made at the first area call of a plan (capture: run the call once before; a captured graph is valid
 * for the rectangle it captured). */
typedef struct j2k_rect { int32_t x0, y0, x1, y1; } j2k_rect;
int j2k_plan_area_shape(const j2k_plan *plan, const j2k_rect *area, int reduce, int *out_w, int *out_h);
int j2k_plan_area_blocks(j2k_plan *plan, const j2k_rect *area, int reduce, uint8_t *d_need);
int j2k_plan_decode_frame_pixels_area(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                      int layers, int truncated, int reduce, int skip_planes, const j2k_rect *area, void *d_pix, size_t stride);
int j2k_decode_pixels_host_area(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int layers, int truncated, int reduce,
                                int skip_planes, const j2k_rect *area, void *pix, size_t stride);

/* Region-of-interest encode (the library's own; the reference has nothing usable here): a rectangle of the frame that the rate control of the
 * closed-loop MQ codec favours.  `roi` is half-open, in full-resolution frame coordinates, as `area` above; `roi_gain` = g is an integer in
 * 1 ... 65535.  Not Maxshift and no change of format: the distortion of the coefficients that reconstruct the rectangle counts g times in the
 * blocks' distortion tables, and the allocation of the budget(s) does the rest.  Streams, packets and every decoder are as before: read such a
 * stream with the _rate / _layers decode calls like any other, and with `area` = the same rectangle.  The decoder is not told.
 *   The rule (definition: tests/roi_cases.py).  Per tile the rectangle is cut to the tile; its need rectangles at reduce = 0 (the
 * region decode's, margins 1 for the 5-3 and 2 for the 9-7) are its footprint in the plane.  A block lies in one band and a band has one need
 * rectangle, so the footprint inside block j is one window F_j, possibly empty.  d_dist[j * 32 + p] = D[p] + (g - 1) * D_in[p] mod 2^64, D the
 * table of j2k_plan_encode_blocks_planes and D_in the same sum over F_j alone: g = 1 or no footprint gives D, a block wholly inside g * D.
 * g weights energy: g = 4^s gives the rectangle about s bit planes of priority; with 8- to 16-bit sources every product stays far below 2^53,
 * so the allocation's float64 slopes see exact integers.  d_rate, the band weights, the hull, the bisection and the packets are untouched.
 *   j2k_plan_roi_windows               d_win[4 j ...] = (fx, fy, fw, fh) of F_j relative to block j's window, all 0 when empty (device int32,
 *                                      4 per job; asynchronous)
 *   j2k_plan_encode_blocks_planes_roi  j2k_plan_encode_blocks_planes with the table above in d_dist (slots, lens, numbps, rate: identical)
 *   j2k_plan_encode_frame_pixels_roi   the frame call for both budget forms: nlayers = 1 with d_layer_offs = NULL writes the stream of
 *                                      j2k_plan_encode_frame_pixels_rate for max_body_bytes = layer_bytes[0]; with d_layer_offs it is
 *                                      j2k_plan_encode_frame_pixels_layers.  Only the distortion launch differs: it takes the rectangle and the gain
 *   j2k_encode_pixels_host_roi         its synchronous host-memory form (layer_offs = NULL with nlayers = 1: the single-budget stream)
 * The rectangle and the gain are kernel arguments: no host table per rectangle, no synchronisation; a captured graph is valid for the rectangle
 * and gain it captured (the plan tables of the region decode are made at the first call: run it once before a capture).
 *   J2K_ERR_UNSUPPORTED: what j2k_plan_rate_allocate refuses (HT, no closed loop, batch, blocks above 64 x 64), a plan that is not Mallat (the
 * prefix layout has no spatial footprint below level 0), a shard plan.  J2K_ERR_INVALID_ARG: a rectangle that is inverted, empty or outside the
 * frame, roi_gain outside 1 ... 65535, no budgets, what the _layers call refuses of its budgets, more than one budget without d_layer_offs.
 * Every refusal comes before the first launch.  One rectangle, no mask, no per-coefficient shift; block-granular in effect, since whole bit
 * planes of whole blocks are kept or cut. */
int j2k_plan_roi_windows(j2k_plan *plan, const j2k_rect *roi, int32_t *d_win);
int j2k_plan_encode_blocks_planes_roi(j2k_plan *plan, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps,
                                      uint32_t *d_rate, uint64_t *d_dist, const j2k_rect *roi, int roi_gain);
int j2k_plan_encode_frame_pixels_roi(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                     const int64_t *layer_bytes, int nlayers, const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap,
                                     uint64_t *d_tile_offs, uint64_t *d_layer_offs);
int j2k_encode_pixels_host_roi(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes,
                               int nlayers, const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len,
                               uint64_t *tile_offs, uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps);

/* Quality-targeted encode (the library's own): the dual of the rate calls above -- "at least this good, in as few bytes as that takes".  The
 * tables, the band weights, the hulls and the rule "block j keeps the last hull point whose slope is >= lambda" are those of
 * j2k_plan_rate_allocate; the search runs on the weighted distortion S = sum_j w_j * float64(d_dist[j * 32 + kept_j]) instead of the byte sum:
 * lambda is the float64 with the LARGEST bit pattern in 0 ... 2^63 - 1 whose choice has S <= target (64 bisection steps).  S is a float64 sum in
 * a FIXED order (the allocation's one workgroup of 1024 threads: thread i adds its blocks i, i + 1024, ... from 0.0, six butterfly steps inside
 * each wavefront, the 16 wavefront values in order); tests/quality_cases.py is the definition the device agrees with bit for bit.  lambda = +0.0
 * keeps everything that lowers a block's distortion, where S = 0: no target is infeasible.  A target at or above the distortion of coding nothing
 * codes nothing.
 *   S is an ESTIMATE of the squared error of the frame, not a bound: the weights are synthesis energy gains, so it measures the colour-transformed
 * components (not RGB), in the coefficient domain, without the rounding of the 5-3, the clamp to the sample range or the cross terms between
 * blocks.  Measure what came out with j2k_pixels_sse; docs/KERNEL_NOTES.md has a table of targets against measured PSNR.  Body bytes only: no
 * header bytes are counted or minimised, and cuts are at whole bit planes.
 *   j2k_plan_psnr_distortion           HOST ONLY: *T = N * peak^2 * q^2 / 10^(dB / 10), N = width * height * components, peak = 2^precision - 1,
 *                                      q = the plan's quality on a lossy plan (its coefficients are the transform times quality), 1 on a lossless one
 *   j2k_plan_rate_allocate_quality     targets[l] (host, non-increasing, 1 <= nlayers <= 32) -> d_kept[l * blocks + j], d_chosen[l] = the body
 *                                      bytes, d_achieved[l] = S of layer l's choice (float64, <= targets[l]); one launch
 *   j2k_plan_encode_frame_pixels_quality  the frame call: j2k_plan_encode_frame_pixels_rate (nlayers = 1, d_layer_offs = NULL) or
 *                                      j2k_plan_encode_frame_pixels_layers with that allocation in the place of theirs; roi (nullable) and
 *                                      roi_gain as j2k_plan_encode_frame_pixels_roi; d_achieved (device, nullable): nlayers float64.  Decode with the
 *                                      _rate / _layers decode calls
 *   j2k_encode_pixels_host_quality     its synchronous host-memory form (achieved: host, nullable)
 * Refusals, all before the first launch: what j2k_plan_rate_allocate / the _layers / the _roi calls refuse, with their codes; a target that is
 * negative, NaN or infinite, targets that rise, nlayers outside 1 ... 32, more than one target without d_layer_offs: J2K_ERR_INVALID_ARG. */
int j2k_plan_psnr_distortion(const j2k_plan *plan, double db, double *T);
int j2k_plan_rate_allocate_quality(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, const double *targets,
                                   int nlayers, uint8_t *d_kept, uint64_t *d_chosen, double *d_achieved);
int j2k_plan_encode_frame_pixels_quality(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph, const double *targets,
                                         int nlayers, const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                         uint64_t *d_layer_offs, double *d_achieved);
int j2k_encode_pixels_host_quality(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, const double *targets,
                                   int nlayers, const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs,
                                   uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps, double *achieved);
/* Per-channel sum of squared sample differences of two DEVICE frames in the same pixel format (J2K_PIX_*; 16-bit samples big-endian):
 * d_sums[c] for every channel as stored -- 1 for the gray formats, 4 (alpha included) for the others -- exact in uint64.  Two launches on the
 * context's stream, no atomics; asynchronous. */
int j2k_pixels_sse(j2k_ctx *ctx, int format, const void *d_a, size_t stride_a, const void *d_b, size_t stride_b, int w, int h, uint64_t *d_sums);

/* The block coder's outputs as those tables.  j2k_plan_t2_packets (host table out): one packet per (tile, component,
 * resolution) of the plan in job order (encoder.go:616-673: tile, component, resolution, band, block row, block column), its
 * code-blocks = the plan's jobs of that resolution, tree widths = block columns of its first band; layer as given.
 * j2k_plan_t2_fill_cbs (device, asynchronous): code-block j from d_offs / d_lens / d_numbps of j2k_plan_encode_stream:
 * IncludedInLayers 0, len(Passes) = 3 * numBPS - 2 (the passes EncodeFast5 runs, t1_fast5.go:66-70; HT blocks: 1; empty
 * blocks: 0), ZeroBitPlanes = max(mb - numBPS, 0) -- the reference never fills these fields from real blocks (only its
 * tests build precincts, t2_test.go), so this mapping is this library's. */
int j2k_plan_t2_packets(const j2k_plan *plan, int layer, j2k_t2_dev_packet *packets, size_t cap, size_t *count);
int j2k_plan_t2_fill_cbs(j2k_plan *plan, int mb, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                         j2k_t2_dev_cb *d_cbs);
/* NewTagTree(width, height) (tcd.go:168-197): number of levels and nodes per level (the coder never walks the tree) */
int j2k_tagtree_shape(int width, int height, int32_t *levels, int64_t *level_sizes, size_t cap);

/* TileDecoder.InitTile (tcd.go:240-390; TileEncoder.InitTile :459-500 computes the same tile and component bounds):
 * tile bounds, component bounds after subsampling (ceilDiv), per resolution r its bounds at scale 2^(NumDecompositions - r)
 * and its bands -- LL for r = 0, else HL, LH, HH with the rectangles initBand writes (HL = upper half, LH = left half,
 * HH = lower right quadrant of the RESOLUTION's rectangle, tcd.go:343-361) -- and every band's code-block grid
 * (2^(exp + 2) squares from the band's origin, clipped).  Flat outputs: comps[ncomp], ress[ncomp * (nd + 1)],
 * bands (component-major, resolution, band order), cbs (band by band, row-major); J2K_ERR_CAPACITY with the counts set
 * when a table is too small.  Field ranges: NumDecompositions <= 32, code-block exponents <= 28, subsampling >= 1
 * (beyond them the reference divides by zero: J2K_ERR_GO_PANIC). */
typedef struct j2k_tcd_header {
    uint32_t image_w, image_h, image_x0, image_y0, tile_w, tile_h, tile_x0, tile_y0, num_tiles_x;
    int32_t ncomp;
    const uint8_t *subsampling;          /* SubsamplingX, SubsamplingY per component */
    uint8_t num_decompositions, cb_w_exp, cb_h_exp, pad_[5];
} j2k_tcd_header;
typedef struct j2k_tcd_rect { int32_t x0, y0, x1, y1; } j2k_tcd_rect;
typedef struct j2k_tcd_band { int32_t comp, res, type, cbx, cby, pad_; j2k_tcd_rect r; uint64_t cb0; } j2k_tcd_band;
int j2k_tcd_init_tile(const j2k_tcd_header *h, int tile_index, j2k_tcd_rect *tile, j2k_tcd_rect *comps, j2k_tcd_rect *ress,
                      j2k_tcd_band *bands, size_t band_cap, size_t *nbands, j2k_tcd_rect *cbs, size_t cb_cap, size_t *ncbs);

/* Pass-level rate control: the same cuts at CODING-PASS ends, three times as many steps per block (an opt-in form beside the calls above, which
 * keep their bytes, tables and refusals; definition: tests/pass_cases.py, argument: DESIGN.md 7).  A block of nb = numBPS planes has the cut
 * points q = 0 ... 3 nb - 2: q = 0 keeps nothing, q >= 1 keeps p = (q + 2) / 3 whole planes from the top and s = (q + 2) % 3 further passes of the
 * next plane (s = 1: its SigProp pass, s = 2: SigProp and MagRef) -- the packet header's pass count itself; 3 p - 2 is a whole-plane cut.
 *   d_rate[j * 96 + q]   uint32: bytes of block j's codeword whose decode has every pass up to q right: [0] = 0, [3 nb - 2] = lens[j], non-decreasing,
 *                        the entries above repeat lens[j]; the coder's byte index at the pass end + 5, capped at the length.
 *                        d_rate[j * 96 + 3 p - 2] is j2k_plan_encode_blocks_planes' d_rate[j * 32 + p].
 *   d_dist[j * 96 + q]   uint64: sum (|v| - |w|)^2 in wrapping arithmetic, w = what j2k_plan_decode_blocks_pfloors leaves of v at that cut; 0 at and
 *                        above 3 nb - 2; [3 p - 2] is the plane table's [p].
 *   d_spmask[j * 64 + y] uint64: the samples of row y (bit x) that turned significant in a SigProp pass, not in Cleanup; rows >= h are 0.
 * j2k_plan_encode_blocks_passes            j2k_plan_encode_blocks + the three tables (the same slots, lens and numbps)
 * j2k_plan_rate_allocate_passes            j2k_plan_rate_allocate on the pass tables: d_kept[j] = the pass count q kept of block j (<= 91)
 * j2k_plan_rate_allocate_quality_passes    j2k_plan_rate_allocate_quality for ONE target on the pass tables (the same fixed float64 sum order)
 * j2k_plan_encode_tile_parts_kept_passes   j2k_plan_encode_tile_parts_kept with d_kept[j] = q: body length d_rate[j * 96 + q], q passes in the header,
 *                                          ZeroBitPlanes = 31 - numBPS as before; q = 0: in no layer.  d_kept[j] = 3 numBPS - 2 everywhere gives
 *                                          j2k_plan_encode_tile_parts' bytes.
 * j2k_plan_decode_tile_parts_pfloors       j2k_plan_decode_tile_parts_floors at pass granularity: with p = (passes + 2) / 3, s = (passes + 2) % 3,
 *                                          floor = max(31 - ZeroBitPlanes - p, 0): d_numbps[j] = p + floor, d_pfloors[j] = the passes left
 *                                          undecoded = 3 floor - s (0 where floor = 0).
 * j2k_plan_decode_blocks_pfloors           block j stops f = max(3 skip_planes, d_pfloors[j]) passes short of its last: whole planes down to
 *                                          ceil(f / 3), then the first 3 ceil(f / 3) - f passes of the next plane; every non-zero sample takes the
 *                                          midpoint of what ITS last pass left undecoded.  d_pfloors[j] = 3 k is j2k_plan_decode_blocks_floors with
 *                                          floors[j] = k, bit for bit.  Every block runs on the one-launch kernel (never the plane-stepped forms).
 * j2k_plan_encode_frame_pixels_passes      the frame encoder with pass cuts: target == NULL: at most max_body_bytes of code-block bodies; else the fewest
 *                                          bytes whose weighted distortion is <= *target (host memory; d_achieved, device or NULL: what was reached).
 *                                          A budget that cuts nothing gives j2k_plan_encode_frame_pixels' bytes.
 * j2k_plan_decode_frame_pixels_passes      the frame decoder for such streams: reduce and skip_planes as the _rate call, area (or NULL) as
 *                                          j2k_plan_decode_frame_pixels_area -- all three only edit the block tables, so they compose as there.
 * j2k_encode_pixels_host_passes /          the synchronous host-memory forms; lens / numbps: the UNCUT lengths and plane counts; achieved (or NULL):
 * j2k_decode_pixels_host_passes            one float64 when a target was given
 * The older readers on such a stream: j2k_plan_decode_frame_pixels_rate (truncated) reads p whole planes per block and ignores s -- valid, the
 * bytes of s further passes are a prefix it does not need.
 * J2K_ERR_UNSUPPORTED: whatever j2k_plan_rate_allocate refuses (HT, no closed loop, batch plans, the raw-MagRef style, blocks above 64 x 64).
 * J2K_ERR_INVALID_ARG: a negative budget, a target that is negative or not finite.  Both before anything is launched; under capture the "run the call
 * once before" rule of the _rate calls.  Not built: layers and a region of interest with pass cuts, the pipelined host codec, the plane-stepped
 * decode forms, batch plans, the HT coder. */
int j2k_plan_encode_blocks_passes(j2k_plan *plan, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps,
                                  uint32_t *d_rate, uint64_t *d_dist, uint64_t *d_spmask);
int j2k_plan_rate_allocate_passes(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                                  int64_t max_body_bytes, uint8_t *d_kept, uint64_t *d_chosen);
int j2k_plan_rate_allocate_quality_passes(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                                          double target, uint8_t *d_kept, uint64_t *d_chosen, double *d_achieved);
int j2k_plan_encode_tile_parts_kept_passes(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                           const uint8_t *d_numbps, const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph,
                                           uint8_t *d_out, size_t cap, uint64_t *d_tile_offs);
int j2k_plan_decode_tile_parts_pfloors(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                       uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_pfloors);
int j2k_plan_decode_blocks_pfloors(j2k_plan *plan, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens,
                                   const uint8_t *d_numbps, int skip_planes, const uint8_t *d_pfloors, int32_t *d_decoded);
int j2k_plan_encode_frame_pixels_passes(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                        int64_t max_body_bytes, const double *target, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                        double *d_achieved);
int j2k_plan_decode_frame_pixels_passes(j2k_plan *plan, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                        int reduce, int skip_planes, const j2k_rect *area, void *d_pix, size_t stride);
int j2k_encode_pixels_host_passes(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph, int64_t max_body_bytes,
                                  const double *target, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint32_t *lens,
                                  uint8_t *numbps, double *achieved);
int j2k_decode_pixels_host_passes(j2k_plan *plan, const uint8_t *cs, size_t len, int sop, int eph, int reduce, int skip_planes,
                                  const j2k_rect *area, void *pix, size_t stride);

/* Rate control on batch plans (j2k_params.frame_rows): a budget or a target PER FRAME.  A batch codes every frame exactly as it would be coded
 * alone; rate control on it has one meaning: FRAME f GETS THE CUTS IT WOULD GET ALONE UNDER ITS OWN BUDGET.  With F = height / frame_rows frames
 * and tiles / F tiles per frame, frame f owns the contiguous blocks whose tile is in [f * tiles / F, (f + 1) * tiles / F); the allocation runs the
 * definitions above (tests/rate_cases.py, layer_cases.py, quality_cases.py, pass_cases.py) on that range alone -- the fixed order of the float64
 * sum starts again at every frame's first block -- in ONE launch of F workgroups (tests/frame_rate_cases.py is the definition).  The stream
 * format, the packet writers and every reader are unchanged: they work per tile.
 *   j2k_plan_set_rate_per_frame        an opt-in plan setting (off by default; the idiom of j2k_plan_set_raw_magref).  OFF: every rate, quality, layer
 *                                      and pass call refuses a batch plan as ever (J2K_ERR_UNSUPPORTED, "a batch plan (frame_rows): not built").
 *                                      ON: every one of them accepts it -- the block and allocation stage calls, the kept / layered tile-part
 *                                      writers, the floors / pfloors / layered readers, the frame encode and decode calls, their host forms,
 *                                      j2k_tile_parts_keep_layers -- and a scalar budget, target or ladder applies to EVERY FRAME SEPARATELY.
 *                                      Layouts: d_kept stays [layers][blocks]; d_chosen and d_achieved (and the host forms' achieved) are
 *                                      [layers][F]: entry l * F + f.  j2k_plan_psnr_distortion gives the target of ONE frame (N = width * frame_rows *
 *                                      components).  On a plan of one frame the setting changes no byte and no table of any call (F = 1).
 *                                      Refused: while the context captures, on != 0 / 1: J2K_ERR_INVALID_ARG; a batch plan that is also a shard
 *                                      (tile_first / tile_count: a frame may be partial): J2K_ERR_UNSUPPORTED.  With F > 1 a region of interest
 *                                      (roi) is J2K_ERR_UNSUPPORTED (the footprint tables know one frame); area decodes of a batch stay refused.
 *   j2k_plan_rate_frames               *frames = F with the setting on, 1 with it off
 * A DIFFERENT budget or target for every frame (a rate controller gives each frame what its buffer allows): host arrays of nframes == F entries,
 * read before the call returns -- they reach the kernels by value, so a captured call replays the values it was captured with, and no call gains a
 * host synchronisation.  One layer; pass_cuts != 0: at coding-pass ends (the 96-entry tables).  No limit on F beyond the plan's.
 *   j2k_plan_rate_allocate_frames          j2k_plan_rate_allocate / _passes, frame f under frame_bytes[f]: d_kept[blocks], d_chosen[F]
 *   j2k_plan_rate_allocate_quality_frames  j2k_plan_rate_allocate_quality (one layer) / _quality_passes, frame f under frame_targets[f]: d_achieved[F]
 *   j2k_plan_encode_frame_pixels_rate_frames  the frame encoder: exactly one of frame_bytes and frame_targets non-NULL; d_achieved (device, [F], may be
 *                                          NULL) is written with frame_targets.  The kept-prefix stream: decode with the _rate / _passes decode calls
 *   j2k_encode_pixels_host_rate_frames     its synchronous host-memory form; lens / numbps / tile_offs as j2k_encode_pixels_host_rate, achieved [F]
 * On a plan of a single frame (F = 1, the setting on or off) frame_bytes = {N} is max_body_bytes = N, byte for byte.
 * Refusals, before anything is launched: nframes != F, a negative budget, a target that is negative or not finite, both or neither of the two
 * arrays: J2K_ERR_INVALID_ARG (the entries need not fall or rise: they belong to different frames); a batch plan with the setting off, and
 * whatever else j2k_plan_rate_allocate refuses: J2K_ERR_UNSUPPORTED.  Not built: one budget over all frames of a batch, per-frame ladders
 * ([F][layers]), roi / area on batches, the pipelined host codec, the HT coder. */
int j2k_plan_set_rate_per_frame(j2k_plan *plan, int on);
int j2k_plan_rate_frames(const j2k_plan *plan, int32_t *frames);
int j2k_plan_rate_allocate_frames(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                                  const int64_t *frame_bytes, int nframes, int pass_cuts, uint8_t *d_kept, uint64_t *d_chosen);
int j2k_plan_rate_allocate_quality_frames(j2k_plan *plan, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps,
                                          const double *frame_targets, int nframes, int pass_cuts, uint8_t *d_kept, uint64_t *d_chosen,
                                          double *d_achieved);
int j2k_plan_encode_frame_pixels_rate_frames(j2k_plan *plan, int format, const void *d_pix, size_t stride, int sop, int eph,
                                             const int64_t *frame_bytes, const double *frame_targets, int nframes, int pass_cuts,
                                             uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, double *d_achieved);
int j2k_encode_pixels_host_rate_frames(j2k_plan *plan, int format, const void *pix, size_t stride, int sop, int eph,
                                       const int64_t *frame_bytes, const double *frame_targets, int nframes, int pass_cuts, uint8_t *out,
                                       size_t cap, size_t *out_len, uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps, double *achieved);

#ifdef __cplusplus
}
#endif
#endif
