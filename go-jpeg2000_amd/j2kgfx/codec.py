"""Batched frame pipeline over the plan calls of the C ABI: the device-side mirror of
encoder.preprocess (encoder.go:216-281), encoder.encodeTile's job loop (encoder.go:597-688),
tcd.TileDecoder.DecodeCodeBlock / ApplyInverseDWT (tcd.go:393-437) and the tail of
decoder.decodeTiles (decoder.go:321-348).

torch is used only to own device memory (tensors on `cuda:<ctx.device>`); all kernels are
launched by libj2kgfx on the context's own (non-blocking) HIP stream, which torch's caching allocator
knows nothing about.  With `track_streams=True` (the default) every stage call therefore
  * makes the library stream wait for what torch has queued on its current stream (inputs written by torch ops), and
  * keeps a reference to every tensor handed over until the next `ctx.sync()` (or `ctx.close()`), so that a temporary
    dropped before then -- `plan.decode_blocks(*plan.encode_stream(plan.forward(x)))` -- is not given to another tensor
    while kernels still use it.  (Not `Tensor.record_stream`: the allocator would record an event on the library stream
    when such a tensor is finally freed, possibly after its context -- and the stream -- are gone: a crash at teardown.)
Results are read after `ctx.sync()` (or after ordering torch's stream behind `torch.cuda.ExternalStream(ctx.stream)`).
bench.py passes `track_streams=False`: its buffers live for the whole run and the launching thread has no slack.
"""
import functools
import ctypes as C
import sys

import numpy as np

from . import _lib
from .context import default_context

BLOCK_DTYPE = np.dtype([("plane", "<i4"), ("band", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4")])


def _torch():
    import torch
    return torch


def _stage(fn):
    """A stage call: order the library stream behind torch's current stream first (see the module docstring)."""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        if self.track_streams:
            t = _torch()
            self._ext().wait_stream(t.cuda.current_stream(self.device))
        return fn(self, *a, **k)
    return wrapped


class FramePlan:
    def __init__(self, width, height, ncomp, precision=8, lossless=True, quality=0, num_resolutions=6,
                 cb=(64, 64), tile=(0, 0), coder=_lib.CODER_MQ, is_signed=False, tile_first=0, tile_count=0,
                 ctx=None, track_streams=True, frame_rows=0, closed_loop=False, dequantize=False, mallat=False, raw_magref=False,
                 rate_per_frame=False):
        self.ctx = ctx or default_context()
        self.track_streams = bool(track_streams)
        self._ext_stream = None
        L = self.ctx.L
        self.params = _lib.Params(width=width, height=height, ncomp=ncomp, precision=precision,
                                  is_signed=int(bool(is_signed)), lossless=int(bool(lossless)), quality=quality,
                                  num_resolutions=num_resolutions, cb_w=cb[0], cb_h=cb[1], tile_w=tile[0],
                                  tile_h=tile[1], coder=coder, tile_first=tile_first, tile_count=tile_count,
                                  frame_rows=frame_rows,    # frame_rows > 0: a batch of height / frame_rows frames stacked vertically
                                  # this library's closed-loop mode (not the reference): windows that partition the plane, readable packets;
                                  # mallat (implies it): level l of the transform on the rectangle [0, w_l) x [0, h_l), so the windows are sub-bands
                                  closed_loop=_lib.CLOSED_LOOP_MALLAT if mallat else int(bool(closed_loop)))
        self.mallat = bool(mallat)
        h = C.c_void_p()
        self.ctx.check(L.j2k_plan_create(self.ctx.h, C.byref(self.params), C.byref(h)))
        self.h = h
        info = _lib.PlanInfo()
        self.ctx.check(L.j2k_plan_get_info(self.h, C.byref(info)))
        self.info = info
        self.width, self.height, self.ncomp = width, height, ncomp
        self.device = "cuda:%d" % self.ctx.device
        from .context import register_plan
        register_plan(self)                     # closed by the package's atexit hook if the caller never does
        if dequantize:
            self.set_dequantize(True)
        if raw_magref:
            self.set_raw_magref(True)
        if rate_per_frame:
            self.set_rate_per_frame(True)

    def close(self):
        if getattr(self, "h", None):
            for pipe in list(getattr(self, "_pipes", ())):     # a j2k_pipe keeps a pointer to its plan
                pipe.close()
            if getattr(self.ctx, "h", None):    # (a plan whose context is gone was destroyed with it)
                self.ctx.L.j2k_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    # ---- geometry ---------------------------------------------------------------
    def blocks(self):
        n = int(self.info.blocks)
        out = np.zeros(n, dtype=BLOCK_DTYPE)
        if n:
            self.ctx.check(self.ctx.L.j2k_plan_get_blocks(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out

    def planes(self):
        """(n,7) int64: tile, comp, x0, y0, w, h, coefficient offset."""
        n = int(self.info.planes)
        out = np.zeros((n, 7), dtype=np.int64)
        self.ctx.check(self.ctx.L.j2k_plan_get_planes(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out

    def decoded_offsets(self):
        n = int(self.info.blocks)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self.ctx.check(self.ctx.L.j2k_plan_get_decoded_offsets(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out[:n]

    def ht_decode_leaders(self):
        """(n,) int32, HT plans: the job whose decode may serve job j too under the option ht_dec_dedup (j itself: none)."""
        n = int(self.info.blocks)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self.ctx.check(self.ctx.L.j2k_plan_get_ht_decode_leaders(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out[:n]

    def ht_decode_walk_order(self):
        """((n,) int32, leaders): HT plans: the job of every slot of the decoder's walk stage -- the `leaders` jobs that lead themselves first."""
        n = int(self.info.blocks)
        out = np.zeros(max(n, 1), dtype=np.int32)
        nl = C.c_int32(0)
        self.ctx.check(self.ctx.L.j2k_plan_get_ht_decode_walk_order(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.byref(nl)))
        return out[:n], int(nl.value)

    # ---- device buffers -----------------------------------------------------------
    def empty(self, n, dtype):
        t = _torch()
        return t.empty(max(int(n), 4), dtype=dtype, device=self.device)

    def alloc_coeff(self):
        return self.empty(self.info.coeff_elems, _torch().int32)

    def alloc_frame(self):
        t = _torch()
        return t.empty((self.ncomp, self.height, self.width), dtype=t.int32, device=self.device)

    def _ext(self):
        if self._ext_stream is None:
            self._ext_stream = _torch().cuda.ExternalStream(self.ctx.stream, device=self.device)
        return self._ext_stream

    def _p(self, t):
        if self.track_streams:
            self.ctx.hold(t)                 # alive until the library stream has been synchronised
        return C.c_void_p(t.data_ptr())

    # ---- stages (asynchronous on the ctx stream) ------------------------------------
    @_stage
    def forward(self, frame, coeff=None):
        """encoder.preprocess for every tile-component: frame int32 [C,H,W] -> coefficient buffer."""
        coeff = coeff if coeff is not None else self.alloc_coeff()
        assert frame.is_contiguous() and frame.numel() == self.ncomp * self.height * self.width
        self.ctx.check(self.ctx.L.j2k_plan_forward(self.h, self._p(frame), self._p(coeff)))
        return coeff

    def reduced_shape(self, reduce):
        """Mallat plans: (H_r, W_r) = ceil(H / 2^reduce), ceil(W / 2^reduce) of a decode with reduce=... (j2k_plan_reduced_size)"""
        w, h = C.c_int32(0), C.c_int32(0)
        self.ctx.check(self.ctx.L.j2k_plan_reduced_size(self.h, int(reduce), C.byref(w), C.byref(h)))
        return int(h.value), int(w.value)

    # ---- region decode (Mallat MQ plans; j2k_plan_*_area) -----------------------------------
    @staticmethod
    def _rect(area):
        x0, y0, x1, y1 = (int(v) for v in area)
        return _lib.Rect(x0, y0, x1, y1)

    def area_shape(self, area, reduce=0):
        """(h, w) of what a decode with area=(x0, y0, x1, y1) (half-open, full-resolution frame coordinates) and reduce=... returns: the
        rectangle [ceil(x0 / 2^reduce), ceil(x1 / 2^reduce)) x [ceil(y0 / 2^reduce), ceil(y1 / 2^reduce)) of the reduced frame (j2k_plan_area_shape)"""
        w, h = C.c_int(0), C.c_int(0)
        r = self._rect(area)
        self.ctx.check(self.ctx.L.j2k_plan_area_shape(self.h, C.byref(r), int(reduce), C.byref(w), C.byref(h)))
        return int(h.value), int(w.value)

    @_stage
    def area_blocks(self, area, reduce=0, need=None):
        """device uint8 [blocks]: 1 for every code-block a decode of `area` at `reduce` needs (j2k_plan_area_blocks)"""
        t = _torch()
        n = int(self.info.blocks)
        need = need if need is not None else self.empty(n, t.uint8)
        r = self._rect(area)
        self.ctx.check(self.ctx.L.j2k_plan_area_blocks(self.h, C.byref(r), int(reduce), self._p(need)))
        return need[:n]

    # ---- region-of-interest encode (Mallat closed-loop MQ plans; j2k_plan_*_roi) --------------
    @_stage
    def roi_windows(self, roi, win=None):
        """device int32 [blocks, 4]: (fx, fy, fw, fh), the footprint of roi=(x0, y0, x1, y1) (half-open, full-resolution frame coordinates)
        inside every code-block, relative to the block's window; all 0 where there is none (j2k_plan_roi_windows)"""
        t = _torch()
        n = int(self.info.blocks)
        win = win if win is not None else t.zeros((max(n, 1), 4), dtype=t.int32, device=self.device)
        r = self._rect(roi)
        self.ctx.check(self.ctx.L.j2k_plan_roi_windows(self.h, C.byref(r), self._p(win)))
        return win[:n]

    @_stage
    def inverse(self, coeff, frame=None, reduce=0):
        """reduce > 0 (Mallat plans): stop at level `reduce`, frame = int32 [C, H_r, W_r] (reduced_shape)"""
        if reduce:
            t = _torch()
            frame = frame if frame is not None else t.empty((self.ncomp,) + self.reduced_shape(reduce), dtype=t.int32, device=self.device)
            self.ctx.check(self.ctx.L.j2k_plan_inverse_reduced(self.h, self._p(coeff), int(reduce), self._p(frame)))
            return frame
        frame = frame if frame is not None else self.alloc_frame()
        self.ctx.check(self.ctx.L.j2k_plan_inverse(self.h, self._p(coeff), self._p(frame)))
        return frame

    @_stage
    def forward_rgba8(self, pix, coeff=None):
        """extractImageData + preprocess fused: pix = device uint8 [H, stride] packed RGBA (image.RGBA.Pix)."""
        coeff = coeff if coeff is not None else self.alloc_coeff()
        assert pix.dim() == 2 and pix.shape[0] == self.height and pix.is_contiguous()
        self.ctx.check(self.ctx.L.j2k_plan_forward_rgba8(self.h, self._p(pix), C.c_size_t(int(pix.shape[1])), self._p(coeff)))
        return coeff

    @_stage
    def inverse_rgba8(self, coeff, pix=None):
        """inverse path + createImage (3 components, 8 bit) fused: returns device uint8 [H, W*4] packed RGBA."""
        t = _torch()
        if pix is None:
            pix = t.empty((self.height, self.width * 4), dtype=t.uint8, device=self.device)
        self.ctx.check(self.ctx.L.j2k_plan_inverse_rgba8(self.h, self._p(coeff), self._p(pix), C.c_size_t(int(pix.shape[1]))))
        return pix

    @_stage
    def encode_blocks(self, coeff, slots=None, lens=None, numbps=None, planes=False, roi=None, roi_gain=16, pass_cuts=False):
        """pass_cuts=True (the plans planes=True takes): the tables at coding-pass granularity, int32 / int64 [blocks, 96], and the SigProp masks,
        int64 [blocks, 64] (j2k_plan_encode_blocks_passes) -- returns (slots, lens, numbps, rate, dist, spmask).
        planes=True (closed-loop MQ plans, blocks <= 64 x 64): also the rate and distortion tables of every block, int32 / int64
        [blocks, 32] holding uint32 / uint64 values (j2k_plan_encode_blocks_planes) -- returns (slots, lens, numbps, rate, dist).
        roi=(x0, y0, x1, y1) with planes=True (Mallat plans): the distortion of the samples that reconstruct that rectangle counts roi_gain
        (1 ... 65535) times in dist; everything else is identical (j2k_plan_encode_blocks_planes_roi)"""
        if roi is not None and not planes:
            raise ValueError("encode_blocks: roi= weights the distortion tables -- it needs planes=True")
        t = _torch()
        n = int(self.info.blocks)
        slots = slots if slots is not None else self.empty(self.info.bytes_cap, t.uint8)
        lens = lens if lens is not None else self.empty(n, t.int32)
        numbps = numbps if numbps is not None else self.empty(n, t.uint8)
        if pass_cuts:
            if roi is not None:
                raise ValueError("encode_blocks: pass_cuts together with roi= -- not built")
            rate = t.zeros((max(n, 1), 96), dtype=t.int32, device=self.device)
            dist = t.zeros((max(n, 1), 96), dtype=t.int64, device=self.device)
            spmask = t.zeros((max(n, 1), 64), dtype=t.int64, device=self.device)
            self.ctx.check(self.ctx.L.j2k_plan_encode_blocks_passes(self.h, self._p(coeff), self._p(slots), self._p(lens), self._p(numbps), self._p(rate),
                                                                    self._p(dist), self._p(spmask)))
            return slots, lens, numbps, rate, dist, spmask
        if planes:
            rate = t.zeros((max(n, 1), 32), dtype=t.int32, device=self.device)
            dist = t.zeros((max(n, 1), 32), dtype=t.int64, device=self.device)
            if roi is not None:
                r = self._rect(roi)
                self.ctx.check(self.ctx.L.j2k_plan_encode_blocks_planes_roi(self.h, self._p(coeff), self._p(slots), self._p(lens), self._p(numbps), self._p(rate),
                                                                            self._p(dist), C.byref(r), int(roi_gain)))
                return slots, lens, numbps, rate, dist
            self.ctx.check(self.ctx.L.j2k_plan_encode_blocks_planes(self.h, self._p(coeff), self._p(slots), self._p(lens),
                                                                    self._p(numbps), self._p(rate), self._p(dist)))
            return slots, lens, numbps, rate, dist
        self.ctx.check(self.ctx.L.j2k_plan_encode_blocks(self.h, self._p(coeff), self._p(slots), self._p(lens),
                                                         self._p(numbps)))
        return slots, lens, numbps

    @_stage
    def rate_allocate(self, rate, dist, numbps, max_body_bytes=None, kept=None, chosen=None, pass_cuts=False, frame_bytes=None):
        """frame_bytes=[one budget per frame] in the place of max_body_bytes (batch plans with set_rate_per_frame; a plan of one frame takes [N]):
        frame f is cut under frame_bytes[f] (j2k_plan_rate_allocate_frames).  chosen: int64 [rate_frames], the body bytes of every frame's choice.
        pass_cuts=True: rate / dist are the 96-entry tables of encode_blocks(pass_cuts=True), kept[j] is a pass count (j2k_plan_rate_allocate_passes).
        the planes to keep of every block so that the code-block BODY bytes are at most max_body_bytes (packet and tile-part headers
        come on top): returns (kept uint8 [blocks], chosen int64 [1] = the body bytes of that choice)  (j2k_plan_rate_allocate)"""
        t = _torch()
        n = int(self.info.blocks)
        kept = kept if kept is not None else self.empty(n, t.uint8)
        if (max_body_bytes is None) == (frame_bytes is None):
            raise ValueError("rate_allocate: one of max_body_bytes and frame_bytes=")
        chosen = self._frame_table("rate_allocate", t, chosen, t.int64, 1)
        if frame_bytes is not None:
            arr, F = self._layer_bytes(self._frame_values("rate_allocate: frame_bytes", frame_bytes, int))
            self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_frames(self.h, self._p(rate), self._p(dist), self._p(numbps), arr, F, int(bool(pass_cuts)),
                                                                    self._p(kept), self._p(chosen)))
            return kept, chosen[:F]
        if pass_cuts:
            self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_passes(self.h, self._p(rate), self._p(dist), self._p(numbps), C.c_int64(int(max_body_bytes)),
                                                                    self._p(kept), self._p(chosen)))
            return kept, chosen[:self.rate_frames]
        self.ctx.check(self.ctx.L.j2k_plan_rate_allocate(self.h, self._p(rate), self._p(dist), self._p(numbps), C.c_int64(int(max_body_bytes)),
                                                         self._p(kept), self._p(chosen)))
        return kept, chosen[:self.rate_frames]

    def _layer_bytes(self, layer_bytes):
        b = [int(x) for x in layer_bytes]
        return (C.c_int64 * max(len(b), 1))(*b), len(b)

    @_stage
    def rate_allocate_layers(self, rate, dist, numbps, layer_bytes, kept=None, chosen=None):
        """rate_allocate for L cumulative budgets in one launch: (kept uint8 [L, blocks], chosen int64 [L]; on a batch plan with set_rate_per_frame
        every frame under the same ladder, chosen [L, rate_frames])  (j2k_plan_rate_allocate_layers)"""
        t = _torch()
        n = int(self.info.blocks)
        arr, L = self._layer_bytes(layer_bytes)
        kept = kept if kept is not None else self.empty(max(L, 1) * n, t.uint8)
        chosen = self._frame_table("rate_allocate_layers", t, chosen, t.int64, L)
        self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_layers(self.h, self._p(rate), self._p(dist), self._p(numbps), arr, L, self._p(kept), self._p(chosen)))
        return kept[:L * n].view(L, n), self._frame_shape(chosen, L)

    # ---- quality targets: the dual of the byte budgets (j2k_*_quality; tests/quality_cases.py is the definition) -------
    def psnr_distortion(self, db):
        """the weighted-distortion target T of a PSNR in dB: width * height * ncomp * peak^2 * q^2 / 10^(dB / 10), peak = 2^precision - 1,
        q = the plan's quality on a lossy plan, 1 on a lossless one; on a batch plan with set_rate_per_frame the target of ONE frame
        (frame_rows in the place of height)  (j2k_plan_psnr_distortion; host only)"""
        T = C.c_double(0.0)
        self.ctx.check(self.ctx.L.j2k_plan_psnr_distortion(self.h, C.c_double(float(db)), C.byref(T)))
        return float(T.value)

    @staticmethod
    def _targets(targets):
        t = [float(x) for x in targets]
        return (C.c_double * max(len(t), 1))(*t), len(t)

    def _quality_args(self, who, max_body_bytes, layer_bytes, min_psnr, max_distortion, layer_psnr, layer_distortion):
        """the one quality argument of an encode call -> (targets, layered), or None without one"""
        given = [k for k, v in (("min_psnr", min_psnr), ("max_distortion", max_distortion), ("layer_psnr", layer_psnr), ("layer_distortion", layer_distortion))
                 if v is not None]
        if not given:
            return None
        if len(given) > 1:
            raise ValueError("%s: %s together -- one quality argument" % (who, " and ".join(given)))
        if max_body_bytes is not None or layer_bytes is not None:
            raise ValueError("%s: %s together with a byte budget -- ask for bytes or for quality" % (who, given[0]))
        if min_psnr is not None:
            return [self.psnr_distortion(min_psnr)], False
        if max_distortion is not None:
            return [float(max_distortion)], False
        if layer_psnr is not None:
            return [self.psnr_distortion(d) for d in layer_psnr], True
        return [float(t) for t in layer_distortion], True

    @_stage
    def rate_allocate_quality(self, rate, dist, numbps, targets=None, kept=None, chosen=None, achieved=None, pass_cuts=False, frame_targets=None):
        """frame_targets=[one target per frame] in the place of targets (batch plans with set_rate_per_frame; one layer): frame f is cut under
        frame_targets[f] (j2k_plan_rate_allocate_quality_frames).  On such a plan chosen and achieved are [L, rate_frames].
        pass_cuts=True: ONE target on the 96-entry tables of encode_blocks(pass_cuts=True), kept[0, j] is a pass count
        (j2k_plan_rate_allocate_quality_passes).
        the planes to keep of every block so that the weighted distortion sum_j w_j * dist[j, kept_j] (float64, in the fixed order of
        tests/quality_cases.py) is at most targets[l], in as few body bytes as the hulls allow; targets fall (or stay) layer by layer:
        (kept uint8 [L, blocks], chosen int64 [L] = body bytes, achieved float64 [L] = that sum)  (j2k_plan_rate_allocate_quality)"""
        t = _torch()
        n = int(self.info.blocks)
        if (targets is None) == (frame_targets is None):
            raise ValueError("rate_allocate_quality: one of targets and frame_targets=")
        arr, L = self._targets(targets) if targets is not None else (None, 1)
        kept = kept if kept is not None else self.empty(max(L, 1) * n, t.uint8)
        chosen = self._frame_table("rate_allocate_quality", t, chosen, t.int64, L)
        achieved = self._frame_table("rate_allocate_quality", t, achieved, t.float64, L)
        if frame_targets is not None:
            arr, F = self._targets(self._frame_values("rate_allocate_quality: frame_targets", frame_targets))
            self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_quality_frames(self.h, self._p(rate), self._p(dist), self._p(numbps), arr, F, int(bool(pass_cuts)),
                                                                            self._p(kept), self._p(chosen), self._p(achieved)))
            return kept[:n].view(1, n), self._frame_shape(chosen, 1), self._frame_shape(achieved, 1)
        if pass_cuts:
            if L != 1:
                raise ValueError("rate_allocate_quality: pass_cuts takes one target (layers with pass cuts: not built)")
            self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_quality_passes(self.h, self._p(rate), self._p(dist), self._p(numbps), C.c_double(float(arr[0])),
                                                                            self._p(kept), self._p(chosen), self._p(achieved)))
            return kept[:n].view(1, n), self._frame_shape(chosen, 1), self._frame_shape(achieved, 1)
        self.ctx.check(self.ctx.L.j2k_plan_rate_allocate_quality(self.h, self._p(rate), self._p(dist), self._p(numbps), arr, L, self._p(kept), self._p(chosen),
                                                                 self._p(achieved)))
        return kept[:L * n].view(L, n), self._frame_shape(chosen, L), self._frame_shape(achieved, L)

    def frame_bound_layers(self, nlayers):
        return int(self.ctx.L.j2k_plan_frame_bound_layers(self.h, int(nlayers)))

    def rate_weights(self):
        """float64 [ncomp, num_resolutions, 4]: the weight of every (component, resolution, band) in rate_allocate.  Default on a Mallat
        plan: the band's synthesis energy gain; on other plans 1 (their windows are not sub-bands)."""
        n = C.c_size_t(0)
        self.ctx.check(self.ctx.L.j2k_plan_get_rate_weights(self.h, None, C.c_size_t(0), C.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        self.ctx.check(self.ctx.L.j2k_plan_get_rate_weights(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(n)))
        return out.reshape(self.ncomp, -1, 4)

    def set_rate_weights(self, weights=None):
        """weights: float64 of rate_weights()'s shape, finite and >= 0; None restores the default"""
        if weights is None:
            self.ctx.check(self.ctx.L.j2k_plan_set_rate_weights(self.h, None, C.c_size_t(0)))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self.ctx.check(self.ctx.L.j2k_plan_set_rate_weights(self.h, w.ctypes.data_as(C.c_void_p), C.c_size_t(w.size)))

    def set_decode_coded_rows_only(self, on=True):
        """HT coder: decode_blocks leaves the rows the reference's decoder never writes (y % 4 != 0) untouched -- the pooled
        HTDecoder's behaviour; the caller owns a buffer it zeroed once (j2k_plan_set_decode_coded_rows_only)."""
        self.ctx.check(self.ctx.L.j2k_plan_set_decode_coded_rows_only(self.h, int(bool(on))))

    def set_dequantize(self, on=True):
        """lossy plans: inverse / inverse_rgba8 / inverse_pixels / decode_frame_pixels / decode_pixels_host multiply every int32
        coefficient by 1.0 / Quality first (dwt.Dequantize, fused into the inverse kernels' loads), so that a lossy frame decodes
        to the picture; off (the default) is tcd.ApplyInverseDWT as the reference wrote it (j2k_plan_set_dequantize)."""
        self.ctx.check(self.ctx.L.j2k_plan_set_dequantize(self.h, int(bool(on))))

    def set_raw_magref(self, on=True):
        """MQ plans with blocks of at most 64 x 64: the raw-MagRef coding style for every later block coder call of the plan -- block bodies are
        H | MQ | RAW, the magnitude-refinement decisions bypass the MQ coder (tests/raw_magref_cases.py is the definition).  encode_blocks,
        encode_stream, decode_blocks (skip_planes=), encode_frame_pixels / decode_frame_pixels (reduce=, skip_planes=, area=), encode_frame_image,
        the host forms and captures of the frame calls follow it; planes=True, byte budgets, layers, quality targets, roi=, truncated=, floors=
        and layers= raise J2K_ERR_UNSUPPORTED on such a plan.  Decode a stream with the setting it was coded with (j2k_plan_set_raw_magref)."""
        self.ctx.check(self.ctx.L.j2k_plan_set_raw_magref(self.h, int(bool(on))))

    @property
    def raw_magref(self):
        return bool(self.ctx.L.j2k_plan_get_raw_magref(self.h))

    # ---- batch plans: a budget or a target per frame (j2k_plan_set_rate_per_frame; tests/frame_rate_cases.py is the definition) -------
    def set_rate_per_frame(self, on=True):
        """batch plans (frame_rows): every rate, quality, layer and pass call -- which refuse a batch plan without this -- accepts the plan and
        gives FRAME f THE CUTS IT WOULD GET ALONE: a scalar budget, target or ladder applies to every frame separately.  kept keeps its shape;
        chosen and achieved gain a frame axis: [F] for the one-layer calls, [L, F] for the layered ones (F = rate_frames; with F = 1 the shapes
        and every byte are as without the setting).  psnr_distortion (and so min_psnr= / layer_psnr=) is the target of ONE frame.  frame_bytes= /
        frame_psnr= / frame_distortion= of the encode calls and frame_bytes= / frame_targets= of the allocation calls give every frame its own
        value.  roi= on such a plan with F > 1 and area= on any batch raise J2K_ERR_UNSUPPORTED; the setter refuses a shard of a batch
        (j2k_plan_set_rate_per_frame)."""
        self.ctx.check(self.ctx.L.j2k_plan_set_rate_per_frame(self.h, int(on)))

    @property
    def rate_frames(self):
        """F: the frames a rate call allocates separately -- height / frame_rows with set_rate_per_frame on, else 1 (j2k_plan_rate_frames)"""
        f = C.c_int32(0)
        self.ctx.check(self.ctx.L.j2k_plan_rate_frames(self.h, C.byref(f)))
        return int(f.value)

    def _frame_table(self, who, t, given, dtype, layers):
        """chosen / achieved of an allocation call: `layers` x rate_frames entries (a caller's tensor that is too small: ValueError)"""
        need = max(int(layers), 1) * self.rate_frames
        if given is None:
            return t.zeros(need, dtype=dtype, device=self.device)
        if int(given.numel()) < need:
            raise ValueError("%s: a tensor of %d entries for %d layer(s) x %d frame(s)" % (who, int(given.numel()), max(int(layers), 1), self.rate_frames))
        return given

    def _frame_shape(self, tab, L):
        """[L x F] entries -> [L] on a plan of one frame (the layout it has always had), else [L, F]"""
        F = self.rate_frames
        return tab[:L] if F == 1 else tab[:L * F].view(L, F)

    def _frame_values(self, who, values, kind=float):
        """one value per frame (a sequence of rate_frames entries; anything else: ValueError)"""
        try:
            v = [kind(x) for x in values]
        except TypeError:
            raise ValueError("%s: a sequence with one entry per frame" % who)
        if len(v) != self.rate_frames:
            raise ValueError("%s: %d entries for the plan's %d frame(s) (rate_frames)" % (who, len(v), self.rate_frames))
        return v

    @_stage
    def forward_pixels(self, fmt, pix, coeff=None):
        """extractImageData (+ rescale to the plan's precision) + preprocess: pix = device uint8 [H, stride] in a Go Pix layout."""
        coeff = coeff if coeff is not None else self.alloc_coeff()
        assert pix.dim() == 2 and pix.shape[0] == self.height and pix.is_contiguous()
        self.ctx.check(self.ctx.L.j2k_plan_forward_pixels(self.h, int(fmt), self._p(pix), C.c_size_t(int(pix.shape[1])), self._p(coeff)))
        return coeff

    def pixels_fused(self, fmt, pix, inverse=False):
        """would forward_pixels / inverse_pixels read / write these pixels in the level-0 kernels (True) or stage them (False)?"""
        r = self.ctx.L.j2k_plan_pixels_fused(self.h, int(fmt), self._p(pix), C.c_size_t(int(pix.shape[1])), 1 if inverse else 0)
        if r < 0:
            self.ctx.check(r)
        return bool(r)

    @property
    def scr16(self):
        """does forward_rgba8 of a fused frame hand level 1's input over as 16-bit rows (context option l0_scr16)?"""
        return bool(self.ctx.L.j2k_plan_scr16(self.h) & 1)

    @property
    def scr16_state(self):
        """j2k_plan_scr16: 1 / 2 = the plan allows the 16-bit hand-off forward / inverse, 4 / 8 = its last forward / inverse call took it"""
        return int(self.ctx.L.j2k_plan_scr16(self.h))

    # ---- image.YCbCr / CMYK / Paletted (encoder.go:178-195; j2kgfx.pixels.YCbCr / CMYK / Paletted) ---------------------------
    def mq_forms(self):
        """j2k_plan_mq_forms, (8,) int32: [0] live contexts of this process that have built an MQ plan, [1] blocks per wavefront of the last
        block encode's MQ chains (0: the one-kernel form), [2] its blocks above 64 x 64 went through symbol lists, [3] the last block decode took
        the plane-stepped path, [4] in this form (option t1_dec_lanes), [5] launches of the big-block decoder, [6] the path was wanted and not
        had (stream not 16-byte aligned / no workspace), [7] 0.  Launches nothing."""
        out = np.zeros(8, dtype=np.int32)
        self.ctx.check(self.ctx.L.j2k_plan_mq_forms(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def _img(self, img):
        for a in img.buffers():
            if hasattr(a, "data_ptr"):
                self._p(a)                     # (held like any stage input)
        return img.struct()

    @_stage
    def forward_image(self, img, coeff=None):
        """forward_pixels(PIX_RGBA8) of the image's colours: img's planes = torch uint8 tensors on the device"""
        coeff = coeff if coeff is not None else self.alloc_coeff()
        s = self._img(img)
        self.ctx.check(self.ctx.L.j2k_plan_forward_image(self.h, C.byref(s), self._p(coeff)))
        return coeff

    def image_fused(self, img):
        """would forward_image read this image in the level-0 kernel (True) or stage it through an RGBA8 frame (False)?"""
        s = img.struct()
        r = self.ctx.L.j2k_plan_image_fused(self.h, C.byref(s))
        if r < 0:
            self.ctx.check(r)
        return bool(r)

    @_stage
    def encode_frame_image(self, img, sop=False, eph=False, out=None, tile_offs=None):
        """closed-loop plans: encode_frame_pixels(PIX_RGBA8) of the image's colours -> (out uint8, tile_offs int64[tiles + 1])"""
        t = _torch()
        out = out if out is not None else self.empty(self.frame_bound(), t.uint8)
        tile_offs = tile_offs if tile_offs is not None else self.empty(int(self.info.tiles) + 1, t.int64)[:int(self.info.tiles) + 1]
        s = self._img(img)
        self.ctx.check(self.ctx.L.j2k_plan_encode_frame_image(self.h, C.byref(s), int(bool(sop)), int(bool(eph)), self._p(out),
                                                              C.c_size_t(int(out.numel())), self._p(tile_offs)))
        return out, tile_offs

    def encode_image_host(self, img, sop=False, eph=False, cap=None):
        """img's planes = numpy uint8 (host) -> dict(bytes, tile_offs, lens, numbps) as encode_pixels_host"""
        L = self.ctx.L
        n, nt = int(self.info.blocks), int(self.info.tiles)
        L.j2k_plan_tile_parts_bound.restype = C.c_size_t
        cap = int(cap) if cap is not None else max(self.frame_bound(), int(L.j2k_plan_tile_parts_bound(self.h))) + 64
        out = np.zeros(max(cap, 1), np.uint8)
        toffs = np.zeros(nt + 1, np.uint64); lens = np.zeros(max(n, 1), np.uint32); nbps = np.zeros(max(n, 1), np.uint8)
        olen = C.c_size_t(0)
        s = img.struct()
        st = L.j2k_encode_image_host(self.h, C.byref(s), int(bool(sop)), int(bool(eph)), out.ctypes.data_as(C.c_void_p), C.c_size_t(cap),
                                     C.byref(olen), toffs.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), nbps.ctypes.data_as(C.c_void_p))
        self.encoded_len = olen.value
        self.ctx.check(st)
        return dict(bytes=out[:olen.value].copy(), tile_offs=toffs, lens=lens[:n].copy(), numbps=nbps[:n].copy())

    @_stage
    def inverse_pixels(self, coeff, pix, reduce=0):
        """inverse path + createImage for the plan's component count and precision into pix (device uint8 [H, stride]; reduce > 0: [H_r, stride])."""
        if reduce:
            self.ctx.check(self.ctx.L.j2k_plan_inverse_pixels_reduced(self.h, self._p(coeff), int(reduce), self._p(pix), C.c_size_t(int(pix.shape[1]))))
            return pix
        self.ctx.check(self.ctx.L.j2k_plan_inverse_pixels(self.h, self._p(coeff), self._p(pix), C.c_size_t(int(pix.shape[1]))))
        return pix

    @_stage
    def encode_stream(self, coeff, stream=None, offs=None, lens=None, numbps=None):
        """encode_blocks + compact in one call (one kernel for HT blocks up to 64x64): returns (stream, offs, lens, numbps)."""
        t = _torch()
        n = int(self.info.blocks)
        stream = stream if stream is not None else self.empty(self.info.bytes_cap, t.uint8)
        offs = offs if offs is not None else self.empty(n + 1, t.int64)
        lens = lens if lens is not None else self.empty(n, t.int32)
        numbps = numbps if numbps is not None else self.empty(n, t.uint8)
        self.ctx.check(self.ctx.L.j2k_plan_encode_stream(self.h, self._p(coeff), self._p(stream), self._p(offs), self._p(lens),
                                                         self._p(numbps)))
        return stream, offs, lens, numbps

    def t2_packets(self, layer=0):
        """one packet per (tile-component, resolution) of the plan in job order: numpy table (t2.DEV_PACKET_DTYPE)"""
        from . import t2
        n = C.c_size_t(0)
        st = self.ctx.L.j2k_plan_t2_packets(self.h, int(layer), None, C.c_size_t(0), C.byref(n))
        if st not in (0, -4):
            self.ctx.check(st)
        out = np.zeros(n.value, t2.DEV_PACKET_DTYPE)
        self.ctx.check(self.ctx.L.j2k_plan_t2_packets(self.h, int(layer), out.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n)))
        return out

    @_stage
    def t2_fill_cbs(self, mb, offs, lens, numbps, cbs=None):
        """the block coder's outputs as the packet coder's code-block table (device uint8 [blocks * 24])"""
        t = _torch()
        cbs = cbs if cbs is not None else self.empty(int(self.info.blocks) * 24, t.uint8)
        self.ctx.check(self.ctx.L.j2k_plan_t2_fill_cbs(self.h, int(mb), self._p(offs), self._p(lens), self._p(numbps), self._p(cbs)))
        return cbs

    # ---- the closed-loop frame codec (plans made with closed_loop=True) ----------------------------------------------
    def frame_bound(self):
        self.ctx.L.j2k_plan_frame_bound.restype = C.c_size_t
        return int(self.ctx.L.j2k_plan_frame_bound(self.h))

    @_stage
    def encode_tile_parts(self, stream, offs, lens, numbps, sop=False, eph=False, out=None, tile_offs=None, kept=None, rate=None, layers=None, pass_cuts=False):
        """pass_cuts=True with kept + rate (rate_allocate(pass_cuts=True), encode_blocks(pass_cuts=True)): every block cut after its first kept[j]
        coding passes (j2k_plan_encode_tile_parts_kept_passes; not with layers=: ValueError).
        the block coder's outputs -> SOT | SOD | packets per tile, end to end: (out uint8, tile_offs int64[tiles + 1]).  kept + rate
        (rate_allocate, encode_blocks(planes=True)): every block cut after its first kept[j] bit planes (j2k_plan_encode_tile_parts_kept).
        layers = L with kept [L, blocks] (rate_allocate_layers): the layered stream -> (out, tile_offs, layer_offs int64 [tiles * L])
        (j2k_plan_encode_tile_parts_layers)"""
        t = _torch()
        if pass_cuts and (layers is not None or kept is None or rate is None):
            raise ValueError("encode_tile_parts: pass_cuts takes kept= and rate= and no layers= (layers with pass cuts: not built)")
        if layers is not None:
            nt, L = int(self.info.tiles), int(layers)
            out = out if out is not None else self.empty(self.frame_bound_layers(L) or 64, t.uint8)
            tile_offs = tile_offs if tile_offs is not None else self.empty(nt + 1, t.int64)[:nt + 1]
            layer_offs = self.empty(nt * max(L, 1), t.int64)[:nt * max(L, 1)]
            self.ctx.check(self.ctx.L.j2k_plan_encode_tile_parts_layers(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps), self._p(kept), self._p(rate),
                                                                        L, int(bool(sop)), int(bool(eph)), self._p(out), C.c_size_t(int(out.numel())), self._p(tile_offs),
                                                                        self._p(layer_offs)))
            return out, tile_offs, layer_offs
        out = out if out is not None else self.empty(self.frame_bound(), t.uint8)
        tile_offs = tile_offs if tile_offs is not None else self.empty(int(self.info.tiles) + 1, t.int64)[:int(self.info.tiles) + 1]
        if kept is not None:
            if pass_cuts:
                self.ctx.check(self.ctx.L.j2k_plan_encode_tile_parts_kept_passes(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps), self._p(kept),
                                                                                 self._p(rate), int(bool(sop)), int(bool(eph)), self._p(out),
                                                                                 C.c_size_t(int(out.numel())), self._p(tile_offs)))
                return out, tile_offs
            self.ctx.check(self.ctx.L.j2k_plan_encode_tile_parts_kept(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps), self._p(kept), self._p(rate),
                                                                      int(bool(sop)), int(bool(eph)), self._p(out), C.c_size_t(int(out.numel())), self._p(tile_offs)))
            return out, tile_offs
        self.ctx.check(self.ctx.L.j2k_plan_encode_tile_parts(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps), int(bool(sop)),
                                                             int(bool(eph)), self._p(out), C.c_size_t(int(out.numel())), self._p(tile_offs)))
        return out, tile_offs

    @_stage
    def decode_tile_parts(self, cs, length, tile_offs=None, sop=False, eph=False, offs=None, lens=None, numbps=None, floors=None, layers=None, dense=None,
                          dense_cap=None, pfloors=None):
        """pfloors = True or a device uint8 [blocks] tensor (the plans rate_allocate takes): the stream's blocks may be cut at coding passes -- returns
        (offs, lens, numbps, pfloors), pfloors[j] = the passes block j's header leaves undecoded (j2k_plan_decode_tile_parts_pfloors).
        tile-parts cs[:length] -> (offs, lens, numbps) as decode_blocks takes them (offsets into cs).  floors = True or a device uint8
        [blocks] tensor (MQ plans): also every block's floor, for streams cut at bit planes -- returns (offs, lens, numbps, floors) with
        numbps counted from each block's top plane down to bit 0 (j2k_plan_decode_tile_parts_floors)"""
        t = _torch()
        n = int(self.info.blocks)
        offs = offs if offs is not None else self.empty(n + 1, t.int64)
        lens = lens if lens is not None else self.empty(n, t.int32)
        numbps = numbps if numbps is not None else self.empty(n, t.uint8)
        if pfloors is not None and pfloors is not False:
            if layers is not None or (floors is not None and floors is not False):
                raise ValueError("decode_tile_parts: pfloors= together with layers= or floors=")
            pfloors = self.empty(n, t.uint8) if pfloors is True else pfloors
            self.ctx.check(self.ctx.L.j2k_plan_decode_tile_parts_pfloors(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                                         int(bool(sop)), int(bool(eph)), self._p(offs), self._p(lens), self._p(numbps), self._p(pfloors)))
            return offs, lens, numbps, pfloors
        if layers is not None:
            # the first `layers` layers of a layered stream: every block's segments gathered into a dense buffer -- returns (dense, offs, lens,
            # numbps, floors), offsets into dense; decode_blocks(dense, offs, lens, numbps, floors=floors) (j2k_plan_decode_tile_parts_layers).
            # dense: a caller-owned device uint8 buffer in the place of one of length + 64 bytes, dense_cap: how many of its bytes the call may
            # use (default: all) -- blocks that do not fit are dropped and frame_status() raises J2K_ERR_CAPACITY
            floors = self.empty(n, t.uint8) if floors is None or floors is True or floors is False else floors
            dense = dense if dense is not None else self.empty(int(length) + 64, t.uint8)
            cap = int(dense.numel()) if dense_cap is None else int(dense_cap)
            if cap < 0 or cap > int(dense.numel()):
                raise _lib.J2KError(_lib.ERR_INVALID_ARG, "decode_tile_parts: dense_cap is not within dense")
            self.ctx.check(self.ctx.L.j2k_plan_decode_tile_parts_layers(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                                        int(bool(sop)), int(bool(eph)), int(layers), self._p(dense), C.c_size_t(cap),
                                                                        self._p(offs), self._p(lens), self._p(numbps), self._p(floors)))
            return dense, offs, lens, numbps, floors
        if floors is not None and floors is not False:
            floors = self.empty(n, t.uint8) if floors is True else floors
            self.ctx.check(self.ctx.L.j2k_plan_decode_tile_parts_floors(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                                        int(bool(sop)), int(bool(eph)), self._p(offs), self._p(lens), self._p(numbps), self._p(floors)))
            return offs, lens, numbps, floors
        self.ctx.check(self.ctx.L.j2k_plan_decode_tile_parts(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                             int(bool(sop)), int(bool(eph)), self._p(offs), self._p(lens), self._p(numbps)))
        return offs, lens, numbps

    @_stage
    def place_blocks(self, decoded, coeff=None):
        coeff = coeff if coeff is not None else self.alloc_coeff()
        self.ctx.check(self.ctx.L.j2k_plan_place_blocks(self.h, self._p(decoded), self._p(coeff)))
        return coeff

    def frame_status(self):
        """synchronises; raises what the asynchronous frame calls found since the last call (capacity, malformed input)"""
        self.ctx.check(self.ctx.L.j2k_plan_frame_status(self.h))
        self.ctx.sync()

    def frame_parallel_tiles(self):
        """synchronises; tiles whose packets the decode calls since the last query parsed side by side (SOP + EPH streams)"""
        import ctypes
        n = ctypes.c_long(0)
        self.ctx.check(self.ctx.L.j2k_plan_frame_parallel_tiles(self.h, ctypes.byref(n)))
        return int(n.value)

    # ---- the frame calls: one resolver from keywords to the C entry point, one block of outputs, one call site per signature -------------------------
    def _encode_form(self, who, max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion):
        """the cut an encode call asks for -> (entry-point suffix, budgets / targets array (or the one budget), L, layered, roi rectangle or None)"""
        q = self._quality_args(who, max_body_bytes, layer_bytes, min_psnr, max_distortion, layer_psnr, layer_distortion)
        if q is not None:
            arr, L = self._targets(q[0])
            return "_quality", arr, L, q[1], self._rect(roi) if roi is not None else None
        if roi is not None and max_body_bytes is None and layer_bytes is None:
            raise ValueError("%s: roi= shifts a budget -- give max_body_bytes= or layer_bytes=" % who)
        if max_body_bytes is not None and layer_bytes is not None:
            raise _lib.J2KError(_lib.ERR_INVALID_ARG, "%s: layer_bytes and max_body_bytes together" % who)
        layered = layer_bytes is not None
        if roi is not None:
            arr, L = self._layer_bytes(layer_bytes if layered else [max_body_bytes])
            return "_roi", arr, L, layered, self._rect(roi)
        if layered:
            arr, L = self._layer_bytes(layer_bytes)
            return "_layers", arr, L, True, None
        if max_body_bytes is not None:
            return "_rate", C.c_int64(int(max_body_bytes)), 1, False, None
        return "", None, 1, False, None

    def _pass_cut_args(self, who, max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion, layers=None):
        """pass_cuts=True of an encode call -> (budget int64, target pointer or None): one of max_body_bytes, min_psnr, max_distortion"""
        for k, v in (("layer_bytes", layer_bytes), ("layer_psnr", layer_psnr), ("layer_distortion", layer_distortion), ("roi", roi), ("layers", layers)):
            if v is not None:
                raise ValueError("%s: pass_cuts together with %s= -- not built" % (who, k))
        given = [k for k, v in (("max_body_bytes", max_body_bytes), ("min_psnr", min_psnr), ("max_distortion", max_distortion)) if v is not None]
        if len(given) != 1:
            raise ValueError("%s: pass_cuts takes one of max_body_bytes=, min_psnr=, max_distortion=" % who)
        if max_body_bytes is not None:
            return C.c_int64(int(max_body_bytes)), None
        T = self.psnr_distortion(min_psnr) if min_psnr is not None else float(max_distortion)
        return C.c_int64(0), C.byref(C.c_double(T))

    def _frame_vector_args(self, who, frame_bytes, frame_psnr, frame_distortion, others):
        """frame_bytes= / frame_psnr= / frame_distortion= of an encode call -> None without one, else (int64 array or None, float64 array or None, F);
        `others`: the call's remaining cut arguments by name -- one of them beside a per-frame one is a ValueError"""
        given = [k for k, v in (("frame_bytes", frame_bytes), ("frame_psnr", frame_psnr), ("frame_distortion", frame_distortion)) if v is not None]
        if not given:
            return None
        if len(given) > 1:
            raise ValueError("%s: %s together -- one per-frame argument" % (who, " and ".join(given)))
        for k, v in others:
            if v is not None:
                raise ValueError("%s: %s= together with %s= -- a value per frame stands alone" % (who, given[0], k))
        if frame_bytes is not None:
            arr, F = self._layer_bytes(self._frame_values("%s: frame_bytes" % who, frame_bytes, int))
            return arr, None, F
        if frame_psnr is not None:
            vals = [self.psnr_distortion(d) for d in self._frame_values("%s: frame_psnr" % who, frame_psnr)]
        else:
            vals = self._frame_values("%s: frame_distortion" % who, frame_distortion)
        arr, F = self._targets(vals)
        return None, arr, F

    @staticmethod
    def _encode_args(form, arr, L, rect, roi_gain):
        """what an encode entry point takes between eph and out"""
        rect = C.byref(rect) if rect is not None else None
        return {"": [], "_rate": [arr], "_layers": [arr, L], "_roi": [arr, L, rect, int(roi_gain)], "_quality": [arr, L, rect, int(roi_gain)]}[form]

    @_stage
    def encode_frame_pixels(self, fmt, pix, sop=False, eph=False, out=None, tile_offs=None, max_body_bytes=None, layer_bytes=None, roi=None, roi_gain=16,
                            min_psnr=None, max_distortion=None, layer_psnr=None, layer_distortion=None, pass_cuts=False, frame_bytes=None, frame_psnr=None,
                            frame_distortion=None):
        """Batch plans with set_rate_per_frame: every budget / target below applies to each frame separately, achieved is [rate_frames] (one layer)
        or [L, rate_frames].  frame_bytes=[...] / frame_psnr=[...] / frame_distortion=[...] (one of them, nothing else that cuts beside it:
        ValueError; rate_frames entries; with or without pass_cuts): frame f under ITS value, the kept-prefix stream -> (out, tile_offs) and, with
        a target, achieved [rate_frames]; on a plan of one frame frame_bytes=[N] is max_body_bytes=N (j2k_plan_encode_frame_pixels_rate_frames).
        pass_cuts=True with one of max_body_bytes, min_psnr, max_distortion (anything else beside it: ValueError): the same stream with every block
        cut at a coding-pass end, not only at a bit-plane end -- about three times as many steps per block (j2k_plan_encode_frame_pixels_passes);
        returns as without it; decode with pass_cuts=True (truncated=True reads the whole planes of it).
        pixels (a Go Pix layout, device uint8 [H, stride]) -> tile-parts: (out uint8, tile_offs int64[tiles + 1]).  max_body_bytes (closed-loop
        MQ plans): at most that many bytes of code-block bodies -- packet and tile-part headers come on top, tile_offs[-1] says what the frame took
        (j2k_plan_encode_frame_pixels_rate); decode with truncated=True.  layer_bytes = [B_0 <= B_1 <= ...] (the same plans; not together with
        max_body_bytes): ONE stream of len(layer_bytes) quality layers, layer l cut as max_body_bytes = B_l would -> (out, tile_offs, layer_offs
        int64 [tiles * L], where every layer of every tile ends) (j2k_plan_encode_frame_pixels_layers); decode with layers=k.
        roi=(x0, y0, x1, y1) with either budget (Mallat plans): a region of interest -- the distortion of the coefficients that reconstruct that
        rectangle counts roi_gain times (an integer 1 ... 65535, a weight on energy: 4^s is about s bit planes of priority), so the budget
        goes there first.  The stream and its decoders are as without it; decode with area=roi for the rectangle alone
        (j2k_plan_encode_frame_pixels_roi).  roi=None takes the calls it took before.
        Quality in the place of bytes (the same plans; one of them, and no byte budget beside it -- ValueError): min_psnr = dB or max_distortion = T
        -> (out, tile_offs, achieved float64 [1]), the stream of max_body_bytes for the fewest body bytes whose weighted distortion estimate is at
        most T = psnr_distortion(dB); layer_psnr = [rising dB] or layer_distortion = [falling T] -> (out, tile_offs, layer_offs, achieved [L]), the
        layered stream.  achieved: the estimate of every layer's choice, <= its target.  An ESTIMATE in the coefficient domain:
        measure the decoded frame with pixels.psnr.  roi= / roi_gain= weigh the rectangle as with a budget (j2k_plan_encode_frame_pixels_quality)"""
        t = _torch()
        fv = self._frame_vector_args("encode_frame_pixels", frame_bytes, frame_psnr, frame_distortion,
                                     (("max_body_bytes", max_body_bytes), ("layer_bytes", layer_bytes), ("roi", roi), ("min_psnr", min_psnr), ("max_distortion", max_distortion),
                                      ("layer_psnr", layer_psnr), ("layer_distortion", layer_distortion)))
        if fv is not None:
            fb, ft, F = fv
            out = out if out is not None else self.empty(self.frame_bound(), t.uint8)
            tile_offs = tile_offs if tile_offs is not None else self.empty(int(self.info.tiles) + 1, t.int64)[:int(self.info.tiles) + 1]
            achieved = t.zeros(F, dtype=t.float64, device=self.device) if ft is not None else None
            self.ctx.check(self.ctx.L.j2k_plan_encode_frame_pixels_rate_frames(self.h, int(fmt), self._p(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)),
                                                                               fb, ft, F, int(bool(pass_cuts)), self._p(out), C.c_size_t(int(out.numel())),
                                                                               self._p(tile_offs), self._p(achieved) if achieved is not None else None))
            return (out, tile_offs) + ((achieved,) if achieved is not None else ())
        F = self.rate_frames
        if pass_cuts:
            budget, target = self._pass_cut_args("encode_frame_pixels", max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion)
            out = out if out is not None else self.empty(self.frame_bound(), t.uint8)
            tile_offs = tile_offs if tile_offs is not None else self.empty(int(self.info.tiles) + 1, t.int64)[:int(self.info.tiles) + 1]
            achieved = t.zeros(F, dtype=t.float64, device=self.device) if target is not None else None
            self.ctx.check(self.ctx.L.j2k_plan_encode_frame_pixels_passes(self.h, int(fmt), self._p(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)),
                                                                          budget, target, self._p(out), C.c_size_t(int(out.numel())), self._p(tile_offs),
                                                                          self._p(achieved) if achieved is not None else None))
            return (out, tile_offs) + ((achieved,) if achieved is not None else ())
        form, arr, L, layered, rect = self._encode_form("encode_frame_pixels", max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion)
        nt = int(self.info.tiles)
        out = out if out is not None else self.empty((self.frame_bound_layers(L) or 64) if layered else self.frame_bound(), t.uint8)
        tile_offs = tile_offs if tile_offs is not None else self.empty(nt + 1, t.int64)[:nt + 1]
        layer_offs = self.empty(nt * max(L, 1), t.int64)[:nt * max(L, 1)] if layered else None
        achieved = t.zeros(max(L, 1) * F, dtype=t.float64, device=self.device) if form == "_quality" else None
        tail = [self._p(out), C.c_size_t(int(out.numel())), self._p(tile_offs)]
        if form in ("_layers", "_roi", "_quality"):
            tail.append(self._p(layer_offs) if layered else None)
        if form == "_quality":
            tail.append(self._p(achieved))
        self.ctx.check(getattr(self.ctx.L, "j2k_plan_encode_frame_pixels" + form)(self.h, int(fmt), self._p(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)),
                                                                                 *(self._encode_args(form, arr, L, rect, roi_gain) + tail)))
        if form == "_quality":          # [L] on a plan of one frame as ever; a batch: [F] for the one target, [L, F] for a ladder
            achieved = achieved[:L] if F == 1 else (achieved[:L * F].view(L, F) if layered else achieved[:F])
        return (out, tile_offs) + ((layer_offs,) if layered else ()) + ((achieved,) if form == "_quality" else ())

    def _decode_form(self, reduce, skip_planes, truncated, layers, area):
        """the decode a call asks for -> (entry-point suffix, what it takes between eph and pix); `area`: a _lib.Rect or None"""
        if area is not None:
            return "_area", [int(layers or 0), int(bool(truncated)), int(reduce), int(skip_planes), C.byref(area)]
        if layers is not None:                   # a layered stream, its first `layers` layers
            return "_layers", [int(layers), int(reduce), int(skip_planes)]
        if truncated:
            return "_rate", [int(reduce), int(skip_planes)]
        if skip_planes:
            return "_coarse", [int(reduce), int(skip_planes)]
        return ("_reduced", [int(reduce)]) if reduce else ("", [])

    @_stage
    def decode_frame_pixels(self, cs, length, pix, tile_offs=None, sop=False, eph=False, reduce=0, skip_planes=0, truncated=False, layers=None, area=None,
                            pass_cuts=False):
        """pass_cuts=True (implies truncated; not with layers=: ValueError): the stream's blocks may be cut at coding passes
        (encode_frame_pixels(pass_cuts=True)); reduce, skip_planes and area compose as with truncated=True (j2k_plan_decode_frame_pixels_passes).
        tile-parts cs[:length] -> pixels into pix (device uint8 [H, stride]; reduce > 0, Mallat plans: [H_r, stride], and only the
        code-blocks of the resolutions it needs are decoded; skip_planes = k > 0, MQ plans: every block decoder stops after bit plane k;
        truncated=True, MQ plans: the stream's blocks may be cut at bit planes (encode_frame_pixels(max_body_bytes=...)) -- every block runs
        from its own top plane down to max(skip_planes, its floor) (j2k_plan_decode_frame_pixels_rate).  Without it a cut stream decodes by
        the old rule, numbps = coded planes.)  layers = k: cs is a layered stream (encode_frame_pixels(layer_bytes=...)); the first k layers of
        every tile-part are read, what follows them is ignored (j2k_plan_decode_frame_pixels_layers).  area = (x0, y0, x1, y1), Mallat MQ plans,
        with any of the others: only that rectangle, pix = [h, stride] with (h, w) = area_shape(area, reduce), and only the code-blocks the
        rectangle needs are decoded (j2k_plan_decode_frame_pixels_area)"""
        rect = self._rect(area) if area is not None else None
        if area is not None and (pix.dim() != 2 or int(pix.shape[0]) != self.area_shape(area, reduce)[0]):
            raise _lib.J2KError(_lib.ERR_INVALID_ARG, "decode_frame_pixels: pix is not area_shape(area, reduce) rows")
        if pass_cuts:
            if layers is not None:
                raise ValueError("decode_frame_pixels: pass_cuts together with layers= -- not built")
            self.ctx.check(self.ctx.L.j2k_plan_decode_frame_pixels_passes(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                                          int(bool(sop)), int(bool(eph)), int(reduce), int(skip_planes),
                                                                          C.byref(rect) if rect is not None else None, self._p(pix), C.c_size_t(int(pix.shape[1]))))
            return pix
        form, args = self._decode_form(reduce, skip_planes, truncated, layers, rect)
        self.ctx.check(getattr(self.ctx.L, "j2k_plan_decode_frame_pixels" + form)(self.h, self._p(cs), C.c_size_t(int(length)), self._p(tile_offs) if tile_offs is not None else None,
                                                                                 int(bool(sop)), int(bool(eph)), *(args + [self._p(pix), C.c_size_t(int(pix.shape[1]))])))
        return pix

    # ---- host memory in, host memory out: the one-call forms (j2k_encode_pixels_host / j2k_decode_pixels_host) -------------------
    def encode_pixels_host(self, fmt, pix, sop=False, eph=False, cap=None, max_body_bytes=None, layer_bytes=None, roi=None, roi_gain=16,
                           min_psnr=None, max_distortion=None, layer_psnr=None, layer_distortion=None, pass_cuts=False, frame_bytes=None, frame_psnr=None,
                           frame_distortion=None):
        """Batch plans with set_rate_per_frame, frame_bytes= / frame_psnr= / frame_distortion=: as encode_frame_pixels (j2k_encode_pixels_host_rate_frames);
        achieved is float64 [rate_frames] for one layer, [L, rate_frames] for a ladder.
        pass_cuts=True: as encode_frame_pixels (j2k_encode_pixels_host_passes); the dict holds achieved float64 [1] when a target was given.
        pix: numpy uint8 [H, stride] (a Go Pix layout) -> dict(bytes, tile_offs, lens, numbps): every tile as a tile-part.  max_body_bytes: as
        encode_frame_pixels (j2k_encode_pixels_host_rate; lens / numbps are the uncut ones); layer_bytes: as encode_frame_pixels, the dict also
        holds layer_offs uint64 [tiles * L] (j2k_encode_pixels_host_layers); roi, roi_gain with either budget: as encode_frame_pixels
        (j2k_encode_pixels_host_roi); min_psnr / max_distortion / layer_psnr / layer_distortion: as encode_frame_pixels, the dict also holds
        achieved float64 [L] (j2k_encode_pixels_host_quality)"""
        L = self.ctx.L
        n, nt = int(self.info.blocks), int(self.info.tiles)
        F = self.rate_frames
        fv = self._frame_vector_args("encode_pixels_host", frame_bytes, frame_psnr, frame_distortion,
                                     (("max_body_bytes", max_body_bytes), ("layer_bytes", layer_bytes), ("roi", roi), ("min_psnr", min_psnr), ("max_distortion", max_distortion),
                                      ("layer_psnr", layer_psnr), ("layer_distortion", layer_distortion)))
        if fv is not None:
            fb, ft, F = fv
            cap = int(cap) if cap is not None else self.frame_bound() + 64
            pix = np.ascontiguousarray(pix, dtype=np.uint8)
            out = np.zeros(max(cap, 1), np.uint8)
            toffs = np.zeros(nt + 1, np.uint64)
            lens = np.zeros(max(n, 1), np.uint32); nbps = np.zeros(max(n, 1), np.uint8)
            ach = np.zeros(F, np.float64)
            olen = C.c_size_t(0)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            st = L.j2k_encode_pixels_host_rate_frames(self.h, int(fmt), ptr(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)), fb, ft, F,
                                                      int(bool(pass_cuts)), ptr(out), C.c_size_t(cap), C.byref(olen), ptr(toffs), ptr(lens), ptr(nbps),
                                                      ptr(ach) if ft is not None else None)
            self.encoded_len = olen.value
            self.ctx.check(st)
            res = dict(bytes=out[:olen.value].copy(), tile_offs=toffs, lens=lens[:n].copy(), numbps=nbps[:n].copy())
            if ft is not None:
                res["achieved"] = ach.copy()
            return res
        if pass_cuts:
            budget, target = self._pass_cut_args("encode_pixels_host", max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion)
            cap = int(cap) if cap is not None else self.frame_bound() + 64
            pix = np.ascontiguousarray(pix, dtype=np.uint8)
            out = np.zeros(max(cap, 1), np.uint8)
            toffs = np.zeros(nt + 1, np.uint64)
            lens = np.zeros(max(n, 1), np.uint32); nbps = np.zeros(max(n, 1), np.uint8)
            ach = np.zeros(F, np.float64)
            olen = C.c_size_t(0)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            st = L.j2k_encode_pixels_host_passes(self.h, int(fmt), ptr(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)), budget, target,
                                                 ptr(out), C.c_size_t(cap), C.byref(olen), ptr(toffs), ptr(lens), ptr(nbps), ptr(ach) if target is not None else None)
            self.encoded_len = olen.value
            self.ctx.check(st)
            res = dict(bytes=out[:olen.value].copy(), tile_offs=toffs, lens=lens[:n].copy(), numbps=nbps[:n].copy())
            if target is not None:
                res["achieved"] = ach.copy()
            return res
        form, arr, nl, layered, rect = self._encode_form("encode_pixels_host", max_body_bytes, layer_bytes, roi, min_psnr, max_distortion, layer_psnr, layer_distortion)
        if cap is None:
            L.j2k_plan_tile_parts_bound.restype = C.c_size_t
            cap = {"_layers": self.frame_bound_layers(nl) or 64, "_roi": max(self.frame_bound_layers(nl) or 64, self.frame_bound()),
                   "_quality": max(self.frame_bound_layers(nl) or 64, self.frame_bound())}.get(form) or max(self.frame_bound(), int(L.j2k_plan_tile_parts_bound(self.h)))
            cap += 64
        cap = int(cap)
        pix = np.ascontiguousarray(pix, dtype=np.uint8)
        out = np.zeros(max(cap, 1), np.uint8)
        toffs = np.zeros(nt + 1, np.uint64); loffs = np.zeros(max(nt * nl, 1), np.uint64)
        lens = np.zeros(max(n, 1), np.uint32); nbps = np.zeros(max(n, 1), np.uint8)
        ach = np.zeros(max(nl, 1) * F, np.float64)
        olen = C.c_size_t(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        tail = [ptr(out), C.c_size_t(cap), C.byref(olen), ptr(toffs)]
        if form in ("_layers", "_roi", "_quality"):
            tail.append(ptr(loffs) if layered else None)
        tail += [ptr(lens), ptr(nbps)] + ([ptr(ach)] if form == "_quality" else [])
        st = getattr(L, "j2k_encode_pixels_host" + form)(self.h, int(fmt), ptr(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)),
                                                        *(self._encode_args(form, arr, nl, rect, roi_gain) + tail))
        self.encoded_len = olen.value
        self.ctx.check(st)
        res = dict(bytes=out[:olen.value].copy(), tile_offs=toffs, lens=lens[:n].copy(), numbps=nbps[:n].copy())
        if form == "_quality":
            res["achieved"] = ach[:nl].copy() if F == 1 else (ach[:nl * F].reshape(nl, F).copy() if layered else ach[:F].copy())
        if layered:
            res["layer_offs"] = loffs[:nt * nl].copy()
        return res

    def decode_pixels_host(self, cs, shape, sop=False, eph=False, reduce=0, skip_planes=0, truncated=False, layers=None, area=None, pix=None, pass_cuts=False):
        """pass_cuts=True: as decode_frame_pixels (j2k_decode_pixels_host_passes).
        closed-loop plans: tile-parts (bytes / numpy uint8) -> numpy uint8 pixels of `shape` = (H, stride); reduce > 0: (H_r, stride);
        skip_planes > 0 (MQ plans), truncated: as decode_frame_pixels; area: as decode_frame_pixels, shape = (h, stride) with h of area_shape
        (j2k_decode_pixels_host_area; pix: a numpy uint8 array of `shape` to write instead of a new one -- a refused call leaves it alone)"""
        cs = np.ascontiguousarray(np.frombuffer(bytes(cs), np.uint8) if not isinstance(cs, np.ndarray) else cs, dtype=np.uint8)
        rect = self._rect(area) if area is not None else None
        if area is not None:
            if len(shape) != 2 or int(shape[0]) != self.area_shape(area, reduce)[0]:
                raise _lib.J2KError(_lib.ERR_INVALID_ARG, "decode_pixels_host: shape is not area_shape(area, reduce) rows")
            pix = pix if pix is not None else np.zeros(shape, np.uint8)
            assert pix.dtype == np.uint8 and pix.shape == tuple(shape) and pix.flags.c_contiguous
        else:
            pix = np.zeros(shape, np.uint8)
        if pass_cuts:
            if layers is not None:
                raise ValueError("decode_pixels_host: pass_cuts together with layers= -- not built")
            self.ctx.check(self.ctx.L.j2k_decode_pixels_host_passes(self.h, cs.ctypes.data_as(C.c_void_p), C.c_size_t(cs.size), int(bool(sop)), int(bool(eph)), int(reduce),
                                                                    int(skip_planes), C.byref(rect) if rect is not None else None, pix.ctypes.data_as(C.c_void_p),
                                                                    C.c_size_t(int(shape[1]))))
            return pix
        form, args = self._decode_form(reduce, skip_planes, truncated, layers, rect)
        self.ctx.check(getattr(self.ctx.L, "j2k_decode_pixels_host" + form)(self.h, cs.ctypes.data_as(C.c_void_p), C.c_size_t(cs.size), int(bool(sop)), int(bool(eph)),
                                                                           *(args + [pix.ctypes.data_as(C.c_void_p), C.c_size_t(int(shape[1]))])))
        return pix

    def pack_bound(self):
        return int(self.ctx.L.j2k_plan_pack_bound(self.h))

    @_stage
    def pack_stream(self, stream, offs, lens, numbps, pack=None):
        """Transport form (blocks without the reference's MEL zero runs + the per-block arrays) of the stream the LAST
        encode_stream call on this plan produced; the first int64 of the pack is its length in bytes."""
        t = _torch()
        pack = pack if pack is not None else self.empty(self.pack_bound(), t.uint8)
        self.ctx.check(self.ctx.L.j2k_plan_pack_stream(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps),
                                                       self._p(pack)))
        return pack

    @_stage
    def assemble_tiles(self, stream, offs, out=None, out_len=None):
        """encoder.createTileHeader for every tile of this plan's shard, on the device (j2k_plan_assemble_tiles_device):
        (out uint8, out_len int64[1]); out[:out_len] = SOT ... SOD data of tile tile_first, tile_first + 1, ... end to end."""
        t = _torch()
        L = self.ctx.L
        L.j2k_plan_tile_parts_bound.restype = C.c_size_t
        out = out if out is not None else self.empty(int(L.j2k_plan_tile_parts_bound(self.h)), t.uint8)
        out_len = out_len if out_len is not None else self.empty(1, t.int64)
        self.ctx.check(L.j2k_plan_assemble_tiles_device(self.h, self._p(stream), self._p(offs), self._p(out), self._p(out_len)))
        return out, out_len

    @_stage
    def unpack_stream(self, pack, stream=None, offs=None, lens=None, numbps=None):
        """Root side of the gather: pack -> (stream, offs, lens, numbps), byte for byte what encode_stream produced."""
        t = _torch()
        n = int(self.info.blocks)
        stream = stream if stream is not None else self.empty(self.info.bytes_cap, t.uint8)
        offs = offs if offs is not None else self.empty(n + 1, t.int64)
        lens = lens if lens is not None else self.empty(n, t.int32)
        numbps = numbps if numbps is not None else self.empty(n, t.uint8)
        self.ctx.check(self.ctx.L.j2k_plan_unpack_stream(self.h, self._p(pack), C.c_size_t(int(pack.numel())), self._p(stream), self._p(offs),
                                                         self._p(lens), self._p(numbps)))
        return stream, offs, lens, numbps

    @_stage
    def unpack_streams(self, packs, outs):
        """unpack_stream for several packs of this geometry in ONE launch: packs = list of uint8 tensors, outs = list of
        (stream, offs, lens, numbps) tuples to fill.  A pack is foreign input: its tensor length is passed along and
        nothing outside it is read."""
        k = len(packs)
        assert k == len(outs)
        VP = C.c_void_p * k
        cols = list(zip(*outs)) if k else [(), (), (), ()]
        arrs = [VP(*[self._p(t_).value for t_ in col]) for col in ([*packs],) + tuple(cols)]
        sizes = (C.c_size_t * k)(*[int(p_.numel()) for p_ in packs])
        self.ctx.check(self.ctx.L.j2k_plan_unpack_streams(self.h, C.c_int(k), arrs[0], sizes, *arrs[1:]))
        return outs

    @_stage
    def compact(self, slots, lens, offs=None, stream=None):
        t = _torch()
        n = int(self.info.blocks)
        offs = offs if offs is not None else self.empty(n + 1, t.int64)
        stream = stream if stream is not None else self.empty(self.info.bytes_cap, t.uint8)
        self.ctx.check(self.ctx.L.j2k_plan_compact(self.h, self._p(slots), self._p(lens), self._p(offs),
                                                   self._p(stream)))
        return offs, stream

    @_stage
    def decode_blocks(self, stream, offs, lens, numbps, decoded=None, skip_planes=0, floors=None, pfloors=None):
        """pfloors: device uint8 [blocks], block j stops max(3 skip_planes, pfloors[j]) coding passes short of its last (j2k_plan_decode_blocks_pfloors).
        skip_planes = k > 0 (MQ plans): every block's decoder stops after bit plane k (j2k_plan_decode_blocks_coarse); floors: device uint8
        [blocks], block j stops after plane max(skip_planes, floors[j]) (j2k_plan_decode_blocks_floors)"""
        t = _torch()
        decoded = decoded if decoded is not None else self.empty(self.info.decoded_elems, t.int32)
        if pfloors is not None:
            if floors is not None:
                raise ValueError("decode_blocks: floors= and pfloors= together")
            self.ctx.check(self.ctx.L.j2k_plan_decode_blocks_pfloors(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps),
                                                                     int(skip_planes), self._p(pfloors), self._p(decoded)))
            return decoded
        if floors is not None:
            self.ctx.check(self.ctx.L.j2k_plan_decode_blocks_floors(self.h, self._p(stream), self._p(offs), self._p(lens), self._p(numbps),
                                                                    int(skip_planes), self._p(floors), self._p(decoded)))
            return decoded
        if skip_planes:
            self.ctx.check(self.ctx.L.j2k_plan_decode_blocks_coarse(self.h, self._p(stream), self._p(offs), self._p(lens),
                                                                    self._p(numbps), int(skip_planes), self._p(decoded)))
            return decoded
        self.ctx.check(self.ctx.L.j2k_plan_decode_blocks(self.h, self._p(stream), self._p(offs), self._p(lens),
                                                         self._p(numbps), self._p(decoded)))
        return decoded

    # ---- host planes in, bytes out (encoder.preprocess + encodeTile) --------------------
    def encode_frame(self, planes):
        """planes: list of C int32 ndarrays (H*W).  Single tile: planes are overwritten with the
        coefficients like e.componentData.  Returns dict(bytes, lens, numbps, tile_offs, coeff)."""
        n = int(self.info.blocks)
        arr = (C.POINTER(C.c_int32) * len(planes))()
        for i, p in enumerate(planes):
            assert p.dtype == np.int32 and p.flags.c_contiguous and p.size == self.width * self.height
            arr[i] = p.ctypes.data_as(C.POINTER(C.c_int32))
        out = np.zeros(max(int(self.info.bytes_cap), 16), dtype=np.uint8)
        coeff = np.zeros(max(int(self.info.coeff_elems), 4), dtype=np.int32)
        lens = np.zeros(max(n, 1), dtype=np.uint32)
        nbps = np.zeros(max(n, 1), dtype=np.uint8)
        toffs = np.zeros(int(self.info.tiles) + 1, dtype=np.uint64)
        olen = C.c_size_t(0)
        self.ctx.check(self.ctx.L.j2k_encode_frame(
            self.h, arr, coeff.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size),
            C.byref(olen), toffs.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
            nbps.ctypes.data_as(C.c_void_p)))
        return dict(bytes=out[:olen.value].copy(), lens=lens[:n].copy(), numbps=nbps[:n].copy(), tile_offs=toffs,
                    coeff=coeff)


# ---- the pipelined host codec (j2k_pipe_*): encode_pixels_host / decode_pixels_host with frames in flight ----------------------------------
class _PinnedBlock:
    """j2k_host_alloc memory, freed when the last array on it goes"""

    def __init__(self, nbytes):
        self._L = _lib.lib()
        self.ptr = self._L.j2k_host_alloc(C.c_size_t(nbytes))
        if not self.ptr:
            raise _lib.J2KError(_lib.ERR_HIP, "j2k_host_alloc(%d) failed" % nbytes)

    def __del__(self):
        if self.ptr and not sys.is_finalizing():
            self._L.j2k_host_free(C.c_void_p(self.ptr))
            self.ptr = None


def pinned_empty(shape, dtype=np.uint8):
    """a numpy array on pinned host memory (j2k_host_alloc), freed with the array: what a HostPipe copies from / to without staging"""
    dtype = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    block = _PinnedBlock(max(nbytes, 1))
    raw = (C.c_uint8 * max(nbytes, 1)).from_address(block.ptr)
    raw._pinned_block = block                      # (numpy keeps `raw` as the array's base, and `raw` the block)
    return np.frombuffer(raw, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)


class HostPipe:
    """j2k_pipe on a FramePlan: submit_encode / submit_decode return tickets, wait(ticket) returns what encode_pixels_host / decode_pixels_host
    return for that frame (or raises what they raise).  At most `depth` tickets may be un-waited.  While tickets are outstanding the plan and
    its context belong to the pipe.  The pipe keeps references to the submitted buffers until their wait."""

    def __init__(self, plan, depth=2):
        self.plan, self.ctx, self.depth = plan, plan.ctx, int(depth)
        self.h = None
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.j2k_pipe_create(plan.h, int(depth), C.byref(h)))
        self.h = h
        self._frames = {}
        self.encoded_len = 0
        if not hasattr(plan, "_pipes"):
            import weakref
            plan._pipes = weakref.WeakSet()
        plan._pipes.add(self)                      # closed with the plan: a j2k_pipe keeps a pointer to its j2k_plan

    @staticmethod
    def _ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def submit_encode(self, fmt, pix, sop=False, eph=False, cap=None, out=None, tables=True):
        """pix: numpy uint8 [H, stride], pinned (pinned_empty) or not; out: the numpy uint8 array the tile-parts go to (default: a new pageable
        one of `cap` bytes; cap default: the plan's bound); tables=False: tile_offs / lens / numbps are not asked for"""
        plan, L = self.plan, self.ctx.L
        n, nt = int(plan.info.blocks), int(plan.info.tiles)
        if cap is None:
            L.j2k_plan_tile_parts_bound.restype = C.c_size_t
            cap = (out.size if out is not None else max(plan.frame_bound(), int(L.j2k_plan_tile_parts_bound(plan.h))) + 64)
        cap = int(cap)
        assert isinstance(pix, np.ndarray) and pix.dtype == np.uint8 and pix.ndim == 2 and pix.flags.c_contiguous
        if out is None:
            out = np.zeros(max(cap, 1), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= cap
        toffs = np.zeros(nt + 1, np.uint64) if tables else None
        lens = np.zeros(max(n, 1), np.uint32) if tables else None
        nbps = np.zeros(max(n, 1), np.uint8) if tables else None
        t = C.c_uint64(0)
        self.ctx.check(L.j2k_pipe_submit_encode(self.h, int(fmt), self._ptr(pix), C.c_size_t(int(pix.shape[1])), int(bool(sop)), int(bool(eph)), self._ptr(out),
                                                C.c_size_t(cap), self._ptr(toffs), self._ptr(lens), self._ptr(nbps), C.byref(t)))
        self._frames[t.value] = ("encode", pix, out, toffs, lens, nbps)
        return t.value

    def submit_decode(self, cs, pix, sop=False, eph=False):
        """cs: tile-parts (bytes / numpy uint8, pinned or not); pix: the numpy uint8 [H, stride] array to decode into, pinned or not"""
        cs = np.frombuffer(bytes(cs), np.uint8) if not isinstance(cs, np.ndarray) else cs
        assert cs.dtype == np.uint8 and cs.flags.c_contiguous
        assert isinstance(pix, np.ndarray) and pix.dtype == np.uint8 and pix.ndim == 2 and pix.flags.c_contiguous
        t = C.c_uint64(0)
        self.ctx.check(self.ctx.L.j2k_pipe_submit_decode(self.h, self._ptr(cs), C.c_size_t(cs.size), int(bool(sop)), int(bool(eph)), self._ptr(pix),
                                                         C.c_size_t(int(pix.shape[1])), C.byref(t)))
        self._frames[t.value] = ("decode", cs, pix)
        return t.value

    def wait(self, ticket):
        """encode: dict(bytes, tile_offs, lens, numbps) as encode_pixels_host (+ out: the caller's array); decode: the pix array.  A refused frame
        raises J2KError (self.encoded_len then holds *out_len: what the tile-parts take, after J2K_ERR_CAPACITY)"""
        olen = C.c_size_t(0)
        st = self.ctx.L.j2k_pipe_wait(self.h, C.c_uint64(int(ticket)), C.byref(olen))
        frame = self._frames.pop(int(ticket), None)
        self.encoded_len = olen.value
        self.ctx.check(st)
        if frame[0] == "decode":
            return frame[2]
        _, _, out, toffs, lens, nbps = frame
        n = int(self.plan.info.blocks)
        res = dict(bytes=out[:olen.value].copy(), out=out)
        if toffs is not None:
            res.update(tile_offs=toffs, lens=lens[:n].copy(), numbps=nbps[:n].copy())
        return res

    def poll(self, ticket):
        done = C.c_int(0)
        self.ctx.check(self.ctx.L.j2k_pipe_poll(self.h, C.c_uint64(int(ticket)), C.byref(done)))
        return bool(done.value)

    def drain(self):
        self.ctx.check(self.ctx.L.j2k_pipe_drain(self.h))

    def close(self):
        """drains, frees the pipe; the plan is usable by the one-call forms again.  Un-waited tickets are gone."""
        if getattr(self, "h", None):
            if getattr(self.plan, "h", None) and getattr(self.ctx, "h", None):
                self.ctx.L.j2k_pipe_destroy(self.h)
            self.h = None
            self._frames = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass
