// j2k_pipe.cpp -- the pipelined host codec (C ABI of libj2kgfx.so, include/j2kgfx.h: j2k_pipe_*, j2k_host_alloc): j2k_encode_pixels_host /
// j2k_decode_pixels_host with up to `depth` frames in flight, so that one frame's copies run beside another frame's kernels.
//
// The contract.  Every kernel of every frame runs on the context's ONE stream in submission order, through the same launch code as the
// one-call forms (encode_host_launch, plan_decode_frame): the plan's workspaces stay single.  What a copy touches exists once per slot: the
// device pixels, the device tile-parts / codestream with their offsets, and a snapshot of the frame's status words, taken -- and the plan's
// words cleared -- on the stream behind the frame's kernels, so one frame's refusal never reaches the next.  One high-priority stream per copy
// direction, chained to the context's stream by events.  The small results (status, length, tables) come back first; the payload copy is
// queued at its exact length once the length is on the host, inside a later submit, poll or wait, and the next frame's small copy only behind
// it (pipe_ring.h, which holds the bookkeeping, says why).  No threads, no environment, and no allocation in steady state.
#include "j2k_host.h"
#include "pipe_ring.h"

using namespace j2k;

namespace {
struct Grown { void *p = nullptr; size_t bytes = 0; };
struct PipeFrame {                       // what a submit leaves for the pump and the wait
    bool encode = true;
    EncodeRequest eq;                    // (plain forms only so far: a later form is a field of these)
    DecodeRequest dq;
    // encode
    uint8_t *out = nullptr; size_t cap = 0;
    uint64_t *tile_offs = nullptr; uint32_t *lens = nullptr; uint8_t *numbps = nullptr;
    bool out_pinned = false;
    size_t total = 0;
    // decode
    void *pix = nullptr; size_t stride = 0, rowbytes = 0;
    bool pix_pinned = false, direct = false;
    // both
    size_t small_bytes = 0;              // what the small copy carries of the slot's meta block
    bool small_recorded = false, pay_recorded = false;
    int hip_result = J2K_OK;             // a HIP failure met while pumping
};
struct PipeSlot {
    Grown d_pix, d_io;                   // device: pixels (encode input, staged decode output); tile-parts + offsets (encode), codestream (decode)
    uint8_t *d_meta = nullptr, *h_meta = nullptr;      // [status words 16][offsets][lens][numbps][block offsets]: device, and its pinned mirror
    Grown h_in, h_out;                   // the pinned ring for pageable caller memory, made at the first frame that needs it
    hipEvent_t ev_h2d = nullptr, ev_k = nullptr, ev_small = nullptr, ev_pay = nullptr;
    PipeFrame f;
};
}  // namespace

struct j2k_pipe {
    j2k_plan *P = nullptr;
    PipeRing ring;
    PipeSlot slot[PipeRing::MAX_DEPTH];
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    size_t off_offs = 0, off_lens = 0, off_nb = 0, off_boffs = 0, meta_bytes = 0, bound = 0;
};

static inline size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

static int grow_device(j2k_ctx *ctx, Grown &g, size_t need) {        // (the slot is free: nothing queued uses the old buffer)
    if (g.p && g.bytes >= need) return J2K_OK;
    if (g.p) { HIPCHK(ctx, hipFree(g.p)); g.p = nullptr; g.bytes = 0; }
    HIPCHK(ctx, hipMalloc(&g.p, std::max<size_t>(need, 64)));
    g.bytes = std::max<size_t>(need, 64);
    return J2K_OK;
}
static int grow_pinned(j2k_ctx *ctx, Grown &g, size_t need) {
    if (g.p && g.bytes >= need) return J2K_OK;
    if (g.p) { HIPCHK(ctx, hipHostFree(g.p)); g.p = nullptr; g.bytes = 0; }
    HIPCHK(ctx, hipHostMalloc(&g.p, std::max<size_t>(need, 64), hipHostMallocDefault));
    g.bytes = std::max<size_t>(need, 64);
    return J2K_OK;
}
// is p pinned host memory (hipHostMalloc, hipHostRegister)?  A failing query means pageable memory.  dev: its device address, or null
static bool pinned_host(const void *p, void **dev) {
    if (dev) *dev = nullptr;
    if (!p) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeHost) return false;
    if (dev && hipHostGetDevicePointer(dev, const_cast<void *>(p), 0) != hipSuccess) { (void)hipGetLastError(); *dev = nullptr; }
    return true;
}
static bool event_done(hipEvent_t e, bool block, int &hip_result) {
    const hipError_t r = block ? hipEventSynchronize(e) : hipEventQuery(e);
    if (r == hipSuccess) return true;
    (void)hipGetLastError();
    if (r == hipErrorNotReady) return false;
    hip_result = J2K_ERR_HIP;            // the frame's wait reports it
    return true;
}

// the payload copy of a frame whose small results are on the host: tile-parts at their exact length, or a staged frame whose status is clean
static void queue_payload(j2k_pipe *pipe, int s) {
    j2k_plan *P = pipe->P;
    PipeSlot &L = pipe->slot[s];
    PipeFrame &f = L.f;
    const int *st = reinterpret_cast<const int *>(L.h_meta);
    const bool clean = f.hip_result == J2K_OK && st[1] == 0 && (!P->spec.closed_loop || st[0] == 0);
    hipError_t e = hipSuccess;
    if (f.encode) {
        f.total = (size_t)reinterpret_cast<const uint64_t *>(L.h_meta + pipe->off_offs)[P->tile_count];
        if (!clean || !f.total || f.total > f.cap || !f.out || f.total > pipe->bound) return;
        e = hipMemcpyAsync(f.out_pinned ? (void *)f.out : L.h_out.p, L.d_io.p, f.total, hipMemcpyDeviceToHost, pipe->s_d2h);
    } else {
        if (!clean || f.direct) return;
        void *dst = f.pix_pinned ? f.pix : L.h_out.p;
        e = f.rowbytes == f.stride ? hipMemcpyAsync(dst, L.d_pix.p, (size_t)P->spec.H * f.stride, hipMemcpyDeviceToHost, pipe->s_d2h)
                                   : hipMemcpy2DAsync(dst, f.stride, L.d_pix.p, f.stride, f.rowbytes, (size_t)P->spec.H, hipMemcpyDeviceToHost, pipe->s_d2h);
    }
    if (e == hipSuccess) e = hipEventRecord(L.ev_pay, pipe->s_d2h);
    if (e != hipSuccess) { (void)hipGetLastError(); f.hip_result = J2K_ERR_HIP; return; }
    f.pay_recorded = true;
}
// the small copy of a frame whose kernels are queued: the slot's snapshot and tables to the host, on the D2H stream behind the frame's kernels
static void queue_small(j2k_pipe *pipe, int s) {
    PipeSlot &L = pipe->slot[s];
    hipError_t e = hipStreamWaitEvent(pipe->s_d2h, L.ev_k, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(L.h_meta, L.d_meta, L.f.small_bytes, hipMemcpyDeviceToHost, pipe->s_d2h);
    if (e == hipSuccess) e = hipEventRecord(L.ev_small, pipe->s_d2h);
    if (e != hipSuccess) { (void)hipGetLastError(); L.f.hip_result = J2K_ERR_HIP; return; }
    L.f.small_recorded = true;
}
static void pump(j2k_pipe *pipe, uint64_t upto) {
    pipe->ring.pump(upto, [&](int s) { queue_small(pipe, s); },
                    [&](int s, bool block) { return !pipe->slot[s].f.small_recorded || event_done(pipe->slot[s].ev_small, block, pipe->slot[s].f.hip_result); },
                    [&](int s) { queue_payload(pipe, s); });
}

static void free_slot_memory(PipeSlot &L) {
    for (Grown *g : {&L.d_pix, &L.d_io}) if (g->p) (void)hipFree(g->p);
    for (Grown *g : {&L.h_in, &L.h_out}) if (g->p) (void)hipHostFree(g->p);
    if (L.d_meta) (void)hipFree(L.d_meta);
    if (L.h_meta) (void)hipHostFree(L.h_meta);
    for (hipEvent_t e : {L.ev_h2d, L.ev_k, L.ev_small, L.ev_pay}) if (e) (void)hipEventDestroy(e);
    L = PipeSlot();
}

extern "C" void *j2k_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void j2k_host_free(void *p) {
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

extern "C" int j2k_pipe_create(j2k_plan *P, int depth, j2k_pipe **out) {
    graph_note_plan(P);
    if (!P || !out) return J2K_ERR_INVALID_ARG;
    *out = nullptr;
    j2k_ctx *ctx = P->ctx;
    if (depth < 1 || depth > PipeRing::MAX_DEPTH) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_pipe_create: depth outside 1 ... 8");
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_pipe_create while the context captures a graph");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    j2k_pipe *pipe = new j2k_pipe();
    pipe->P = P;
    pipe->ring.init(depth);
    const PlanSpec &S = P->spec;
    const size_t nb = P->blocks.size(), nt = (size_t)P->tile_count;
    pipe->off_offs = 16;
    pipe->off_lens = align16(pipe->off_offs + (nt + 2) * 8);
    pipe->off_nb = align16(pipe->off_lens + nb * 4);
    pipe->off_boffs = align16(pipe->off_nb + nb);
    pipe->meta_bytes = align16(pipe->off_boffs + (nb + 1) * 8);
    pipe->bound = plain_bound(P);
    const size_t pixbytes = (size_t)S.W * S.H * (S.C == 1 ? 1 : 4) * (S.precision > 8 ? 2 : 1);
    int r = J2K_OK;
    auto hip = [&](hipError_t e, const char *what) { if (r == J2K_OK && e != hipSuccess) r = fail_hip(ctx, e, what); };
    int least = 0, greatest = 0;
    hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
    if (r == J2K_OK) hip(hipStreamCreateWithPriority(&pipe->s_h2d, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority");
    if (r == J2K_OK) hip(hipStreamCreateWithPriority(&pipe->s_d2h, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority");
    for (int i = 0; i < depth && r == J2K_OK; i++) {
        PipeSlot &L = pipe->slot[i];
        for (hipEvent_t *e : {&L.ev_h2d, &L.ev_k, &L.ev_small, &L.ev_pay})
            if (r == J2K_OK) hip(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreateWithFlags");
        if (r == J2K_OK) hip(hipMalloc((void **)&L.d_meta, pipe->meta_bytes), "hipMalloc (pipe)");
        if (r == J2K_OK) hip(hipHostMalloc((void **)&L.h_meta, pipe->meta_bytes, hipHostMallocDefault), "hipHostMalloc (pipe)");
        if (r == J2K_OK) r = grow_device(ctx, L.d_io, encode_host_io_bytes(P, false, 1, pipe->bound));
        if (r == J2K_OK) r = grow_device(ctx, L.d_pix, pixbytes);
    }
    if (r != J2K_OK) { j2k_pipe_destroy(pipe); return r; }
    *out = pipe;
    return J2K_OK;
}

extern "C" int j2k_pipe_drain(j2k_pipe *pipe) {
    if (!pipe) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = pipe->P->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pump(pipe, ~uint64_t(0));
    HIPCHK(ctx, hipStreamSynchronize(pipe->s_d2h));
    return J2K_OK;
}

extern "C" void j2k_pipe_destroy(j2k_pipe *pipe) {
    if (!pipe) return;
    (void)hipSetDevice(pipe->P->ctx->device);
    if (pipe->s_d2h) (void)j2k_pipe_drain(pipe);
    (void)hipStreamSynchronize(pipe->P->ctx->stream);
    if (pipe->s_h2d) { (void)hipStreamSynchronize(pipe->s_h2d); (void)hipStreamDestroy(pipe->s_h2d); }
    if (pipe->s_d2h) { (void)hipStreamSynchronize(pipe->s_d2h); (void)hipStreamDestroy(pipe->s_d2h); }
    for (PipeSlot &L : pipe->slot) free_slot_memory(L);
    delete pipe;
}

// what every submit starts with: the pipe, a free slot (else nothing is queued and no ticket consumed), the device, and the payload copies of
// earlier frames whose lengths have arrived
static int submit_begin(j2k_pipe *pipe, int *slot) {
    j2k_ctx *ctx = pipe->P->ctx;
    const int s = pipe->ring.free_slot();
    if (s < 0) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_pipe: `depth` tickets are un-waited");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pump(pipe, 0);
    pipe->slot[s].f = PipeFrame();
    *slot = s;
    return J2K_OK;
}
// a submit that failed after it queued something: the slot stays free, so what was queued must be over before the slot is filled again
static int submit_abort(j2k_pipe *pipe, int r) {
    j2k_ctx *ctx = pipe->P->ctx;
    const std::string msg = ctx->last_error;
    if (hipStreamSynchronize(pipe->s_h2d) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) (void)hipGetLastError();
    ctx->last_error = msg;
    return r;
}
#define PIPECHK(call)                                                              \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) return submit_abort(pipe, fail_hip(ctx, e_, #call)); \
    } while (0)

// host memory -> the slot's device buffer on the H2D stream (pageable memory through the pinned ring), and the context's stream behind it
static int submit_upload(j2k_pipe *pipe, PipeSlot &L, void *d_dst, const void *src, size_t bytes) {
    j2k_ctx *ctx = pipe->P->ctx;
    if (bytes && !pinned_host(src, nullptr)) {
        const int r = grow_pinned(ctx, L.h_in, bytes);
        if (r != J2K_OK) return r;
        memcpy(L.h_in.p, src, bytes);
        src = L.h_in.p;
    }
    if (bytes) PIPECHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, pipe->s_h2d));
    PIPECHK(hipEventRecord(L.ev_h2d, pipe->s_h2d));
    PIPECHK(hipStreamWaitEvent(ctx->stream, L.ev_h2d, 0));
    return J2K_OK;
}
// behind a frame's kernels, on the context's stream: the plan's status word and the block coders' fault word into the slot's snapshot, both
// cleared, and the event the small copy (`bytes` of the slot's meta block, queued by the pump) waits for
static int submit_results(j2k_pipe *pipe, PipeSlot &L, size_t bytes) {
    j2k_plan *P = pipe->P;
    j2k_ctx *ctx = P->ctx;
    if (P->d_frame_status) {
        PIPECHK(hipMemcpyAsync(L.d_meta, P->d_frame_status, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        PIPECHK(hipMemsetAsync(P->d_frame_status, 0, sizeof(int), ctx->stream));
    }
    if (ctx->fault_armed && ctx->stage[3]) {
        PIPECHK(hipMemcpyAsync(L.d_meta + sizeof(int), ctx->stage[3], sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        PIPECHK(hipMemsetAsync(ctx->stage[3], 0, sizeof(int), ctx->stream));
        ctx->fault_armed = false;
    }
    PIPECHK(hipEventRecord(L.ev_k, ctx->stream));
    L.f.small_bytes = bytes;
    return J2K_OK;
}

extern "C" int j2k_pipe_submit_encode(j2k_pipe *pipe, int format, const void *pix, size_t stride, int sop, int eph, uint8_t *out, size_t cap, uint64_t *tile_offs,
                                      uint32_t *lens, uint8_t *numbps, uint64_t *ticket) {
    if (!pipe) return J2K_ERR_INVALID_ARG;
    j2k_plan *P = pipe->P;
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    int r = host_call_check(P, pix, ticket);
    if (r != J2K_OK) return r;
    const int pb = pix_format_bytes(format);
    if (!pb || stride < (size_t)S.W * pb) return fail(ctx, J2K_ERR_INVALID_ARG, "pixel format / stride");
    if (j2k_plan_pixels_fused(P, format, reinterpret_cast<const void *>(uintptr_t(256)), stride, 0) < 0)
        return fail(ctx, J2K_ERR_INVALID_ARG, "pixel format and plan disagree on the component count");
    int s = -1;
    if ((r = submit_begin(pipe, &s)) != J2K_OK) return r;
    PipeSlot &L = pipe->slot[s];
    PipeFrame &f = L.f;
    f.encode = true;
    f.out = out; f.cap = cap; f.tile_offs = tile_offs; f.lens = lens; f.numbps = numbps;
    f.out_pinned = pinned_host(out, nullptr);
    const size_t pixbytes = (size_t)S.H * stride, nb = P->blocks.size();
    if ((r = grow_device(ctx, L.d_pix, pixbytes)) != J2K_OK) return r;
    if (out && !f.out_pinned && (r = grow_pinned(ctx, L.h_out, pipe->bound)) != J2K_OK) return r;
    if ((r = submit_upload(pipe, L, L.d_pix.p, pix, pixbytes)) != J2K_OK) return r;
    HostEncodeIO io;
    void *d_pix = L.d_pix.p;
    r = encode_host_launch(P, f.eq, false, pipe->bound, sop, eph, L.d_io.p, [&](int32_t *d_coeff) { return j2k_plan_forward_pixels(P, format, d_pix, stride, d_coeff); }, io);
    if (r != J2K_OK) return submit_abort(pipe, r);
    // the frame's results into the slot: the offsets always, the tables the caller asked for
    PIPECHK(hipMemsetAsync(L.d_meta, 0, 16, ctx->stream));
    PIPECHK(hipMemcpyAsync(L.d_meta + pipe->off_offs + io.offs_at * 8, io.d_offs, io.offs_count * 8, hipMemcpyDeviceToDevice, ctx->stream));
    const bool boffs = !S.closed_loop && tile_offs;
    if (lens && nb) PIPECHK(hipMemcpyAsync(L.d_meta + pipe->off_lens, io.d_lens, nb * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (numbps && nb) PIPECHK(hipMemcpyAsync(L.d_meta + pipe->off_nb, io.d_numbps, nb, hipMemcpyDeviceToDevice, ctx->stream));
    if (boffs) PIPECHK(hipMemcpyAsync(L.d_meta + pipe->off_boffs, P->d_offs, (nb + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if ((r = submit_results(pipe, L, (lens || numbps || boffs) ? pipe->meta_bytes : pipe->off_lens)) != J2K_OK) return r;
    *ticket = pipe->ring.commit(s);
    pump(pipe, 0);
    return J2K_OK;
}

extern "C" int j2k_pipe_submit_decode(j2k_pipe *pipe, const uint8_t *cs, size_t len, int sop, int eph, void *pix, size_t stride, uint64_t *ticket) {
    if (!pipe) return J2K_ERR_INVALID_ARG;
    j2k_plan *P = pipe->P;
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    int r = host_call_check(P, cs, pix);
    if (r != J2K_OK) return r;
    if (!ticket) return J2K_ERR_INVALID_ARG;
    if (!S.closed_loop) return fail(ctx, J2K_ERR_UNSUPPORTED, "the plan was not made with j2k_params.closed_loop: the reference has no decode body to mirror");
    // what the frame decoder's last stage refuses (j2k_pack_pixels), decided before anything is queued
    if (S.C != 1 && S.C != 3 && S.C != 4) return fail(ctx, J2K_ERR_UNSUPPORTED, "unsupported number of components");
    if (S.precision < 1 || S.precision > 16) return fail(ctx, J2K_ERR_INVALID_ARG, "precision outside 1 ... 16");
    const size_t bps = S.precision > 8 ? 2 : 1, rowbytes = (size_t)S.W * (S.C == 1 ? 1 : 4) * bps;
    if (stride < rowbytes) return fail(ctx, J2K_ERR_INVALID_ARG, "stride smaller than a row");
    const size_t align = S.C == 1 ? bps : 4;         // what the device call takes of a frame's address (RGBA rows: 4 bytes)
    if (S.C != 1 && bps == 1 && (stride & 3)) return fail(ctx, J2K_ERR_INVALID_ARG, "RGBA rows must be 4-byte aligned");
    int s = -1;
    if ((r = submit_begin(pipe, &s)) != J2K_OK) return r;
    PipeSlot &L = pipe->slot[s];
    PipeFrame &f = L.f;
    f.encode = false;
    f.pix = pix; f.stride = stride; f.rowbytes = rowbytes;
    void *d_direct = nullptr;
    f.pix_pinned = pinned_host(pix, &d_direct);
    // a pinned frame is stored by the inverse transform itself, through its device address; one whose address the device call does not take
    // goes through the slot's device frame and a copy, as a pageable one does
    f.direct = f.pix_pinned && d_direct && ((uintptr_t)d_direct & (align - 1)) == 0;
    const size_t pixbytes = (size_t)S.H * stride;
    if ((r = grow_device(ctx, L.d_io, len + 64)) != J2K_OK) return r;
    if (!f.direct && (r = grow_device(ctx, L.d_pix, pixbytes)) != J2K_OK) return r;
    if (!f.pix_pinned && (r = grow_pinned(ctx, L.h_out, pixbytes)) != J2K_OK) return r;
    if ((r = submit_upload(pipe, L, L.d_io.p, cs, len)) != J2K_OK) return r;
    r = plan_decode_frame(P, (const uint8_t *)L.d_io.p, len, nullptr, sop, eph, f.dq, nullptr, f.direct ? d_direct : L.d_pix.p, stride);
    if (r != J2K_OK) return submit_abort(pipe, r);
    PIPECHK(hipMemsetAsync(L.d_meta, 0, 16, ctx->stream));
    if ((r = submit_results(pipe, L, 16)) != J2K_OK) return r;
    *ticket = pipe->ring.commit(s);
    pump(pipe, 0);
    return J2K_OK;
}

extern "C" int j2k_pipe_poll(j2k_pipe *pipe, uint64_t ticket, int *done) {
    if (!pipe || !done) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = pipe->P->ctx;
    *done = 0;
    const int s = pipe->ring.find(ticket);
    if (s < 0) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_pipe_poll: no such un-waited ticket");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pump(pipe, 0);
    PipeSlot &L = pipe->slot[s];
    if (pipe->ring.payload_queued(s)) *done = (!L.f.pay_recorded || event_done(L.ev_pay, false, L.f.hip_result)) ? 1 : 0;
    return J2K_OK;
}

extern "C" int j2k_pipe_wait(j2k_pipe *pipe, uint64_t ticket, size_t *out_len) {
    if (!pipe) return J2K_ERR_INVALID_ARG;
    j2k_plan *P = pipe->P;
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    const int s = pipe->ring.find(ticket);
    if (s < 0) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_pipe_wait: no such un-waited ticket");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pump(pipe, ticket);
    PipeSlot &L = pipe->slot[s];
    PipeFrame &f = L.f;
    if (f.pay_recorded) (void)event_done(L.ev_pay, true, f.hip_result);
    pipe->ring.retire(s, true);
    if (f.hip_result != J2K_OK) return fail(ctx, J2K_ERR_HIP, "j2k_pipe: a copy or an event of this frame failed");
    const int *st = reinterpret_cast<const int *>(L.h_meta);
    int r = fault_result(ctx, st[1]);
    if (r == J2K_OK && S.closed_loop) r = frame_status_result(ctx, st[0]);
    if (r != J2K_OK) return r;
    if (!f.encode) {
        if (!f.direct && !f.pix_pinned)
            for (int y = 0; y < S.H; y++) memcpy((uint8_t *)f.pix + (size_t)y * f.stride, (const uint8_t *)L.h_out.p + (size_t)y * f.stride, f.rowbytes);
        return J2K_OK;
    }
    const size_t nb = P->blocks.size(), nt = (size_t)P->tile_count;
    const uint64_t *offs = reinterpret_cast<const uint64_t *>(L.h_meta + pipe->off_offs);
    if (out_len) *out_len = f.total;
    if (f.tile_offs && S.closed_loop) memcpy(f.tile_offs, offs, (nt + 1) * 8);
    else if (f.tile_offs) reference_tile_offs(P, reinterpret_cast<const uint64_t *>(L.h_meta + pipe->off_boffs), f.total, f.tile_offs);
    if (f.lens && nb) memcpy(f.lens, L.h_meta + pipe->off_lens, nb * 4);
    if (f.numbps && nb) memcpy(f.numbps, L.h_meta + pipe->off_nb, nb);
    if (f.total > f.cap || (f.total && !f.out)) return fail(ctx, J2K_ERR_CAPACITY, "out too small (*out_len says what the tile-parts take)");
    if (f.total && !f.pay_recorded) return fail(ctx, J2K_ERR_HIP, "j2k_pipe: the tile-parts exceed the plan's bound");
    if (f.total && !f.out_pinned) memcpy(f.out, L.h_out.p, f.total);
    return J2K_OK;
}
