"""Characterization of the closed-loop frame calls: every encode form, every decode form, the refusal status of every frame entry point for a table
of bad calls (two faults at once included: the order of the checks is behaviour), and one captured encode and decode -- device method and host
method.  Nothing here says what the right answer is (the other test modules do, against the oracle); this one pins what the calls DID when
tests/frame_forms_recorded.json was written, so that the host layer above the kernels can be rearranged without moving a byte or a status.

    python tests/test_gpu_frame_forms.py        # writes the JSON: run on the commit BEFORE a refactor, never on the code under test

Values are sha256 digests (streams up to tile_offs[-1], the offset tables, `achieved` as raw float64, decoded pixels), or {"status": s} where the
call (or the frame status after it) was refused."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "frame_forms_recorded.json")
MQ, HT = 0, 1
GRAY16, RGBA8 = 1, 2
FILL = 0xA5

# name -> (width, height, components, precision, pixel format, FramePlan keywords, roi rectangle, area rectangle)
A_RECTS = ((40, 30, 90, 70), (50, 20, 80, 75))           # both cross the tile boundaries x = 64 and y = 64
A_KW = dict(lossless=True, num_resolutions=3, cb=(32, 32), tile=(64, 64))
PLANS = {
    "A": (96, 80, 3, 8, RGBA8, dict(A_KW, coder=MQ, mallat=True)) + A_RECTS,
    "B": (80, 96, 1, 12, GRAY16, dict(lossless=False, quality=75, num_resolutions=3, cb=(32, 32), coder=MQ, mallat=True, dequantize=True), (20, 30, 70, 90), (30, 20, 75, 70)),
    "C": (96, 80, 3, 8, RGBA8, dict(A_KW, coder=HT, mallat=True)) + A_RECTS,
    "D": (96, 80, 3, 8, RGBA8, dict(A_KW, coder=MQ, closed_loop=True)) + A_RECTS,
    "E": (96, 80, 3, 8, RGBA8, dict(A_KW, coder=MQ)) + A_RECTS,
    "F": (96, 80, 3, 8, RGBA8, dict(A_KW, coder=MQ, mallat=True, raw_magref=True)) + A_RECTS,
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_pixels(fmt, W, H, seed):
    """a gradient plus low-amplitude noise (so that budgets cut), in the Go Pix layout of `fmt`"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if fmt == RGBA8:
        pix = np.full((H, W, 4), 255, np.uint8)
        for c in range(3):
            pix[:, :, c] = np.clip((2 * x + y + 40 * c) % 256 + rng.integers(-4, 5, size=(H, W)), 0, 255)
        return pix.reshape(H, W * 4)
    v = np.clip((37 * x + 21 * y) % 4096 + rng.integers(-32, 33, size=(H, W)), 0, 4095).astype(np.uint16) << 4      # 12 bits in Gray16 (big-endian)
    return np.stack([(v >> 8).astype(np.uint8), (v & 255).astype(np.uint8)], axis=-1).reshape(H, W * 2)


def make_ycbcr(W, H, seed, to_dev=None):
    from j2kgfx import _lib
    from j2kgfx.pixels import YCbCr
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    Y = np.clip((2 * x + y) % 256 + rng.integers(-4, 5, size=(H, W)), 0, 255).astype(np.uint8).reshape(-1)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    cb = rng.integers(96, 160, size=cw * ch).astype(np.uint8)
    cr = rng.integers(96, 160, size=cw * ch).astype(np.uint8)
    f = to_dev if to_dev is not None else (lambda a: a)
    return YCbCr(f(Y), f(cb), f(cr), W, cw, _lib.YCBCR_420, (0, 0, W, H))


class Env:
    def __init__(self):
        import torch
        from j2kgfx import Context, J2KError, _lib
        from j2kgfx.codec import FramePlan
        self.torch, self.J2KError, self.lib, self.FramePlan = torch, J2KError, _lib, FramePlan
        self.ctx = Context(0)
        self.L = self.ctx.L
        self.out = {}

    def plan(self, name, ctx=None):
        W, H, Cn, prec, fmt, kw = PLANS[name][:6]
        return self.FramePlan(W, H, Cn, precision=prec, ctx=ctx or self.ctx, **kw)

    def run(self, fn):
        try:
            return fn()
        except self.J2KError as e:
            return {"status": int(e.status)}
        except ValueError:
            return {"raises": "ValueError"}

    def close(self):
        self.ctx.close()


# ---- encode and decode forms ----------------------------------------------------------------------------------------------------------------------
def encode_forms(name, body):
    """(form id, keywords) of the encode forms of plan `name`; body = the bytes of the plain frame's code-blocks"""
    roi = PLANS[name][6]
    forms = [("plain", {})]
    if name in "ABD":
        forms += [("rate_half", dict(max_body_bytes=body // 2)), ("rate_all", dict(max_body_bytes=2 * body + 4096)),
                  ("layers3", dict(layer_bytes=[body // 4, body // 2, 3 * body // 4]))]
    if name in "AB":
        forms += [("roi_rate", dict(max_body_bytes=body // 2, roi=roi, roi_gain=16)), ("roi_layers", dict(layer_bytes=[body // 4, body // 2, 3 * body // 4], roi=roi, roi_gain=16)),
                  ("min_psnr", dict(min_psnr=38.0))]
    if name == "A":
        forms += [("layer_psnr", dict(layer_psnr=[32.0, 40.0])), ("layer_psnr_roi", dict(layer_psnr=[32.0, 40.0], roi=roi, roi_gain=16))]
    return forms


def nlayers_of(kw):
    for k in ("layer_bytes", "layer_psnr"):
        if k in kw:
            return len(kw[k])
    return 0


def decode_combos(name, kw):
    area = PLANS[name][7]
    if name == "C":
        return [("plain", {}), ("reduce1", dict(reduce=1))]
    if name == "F":
        return [("plain", {}), ("skip2", dict(skip_planes=2))]
    L = nlayers_of(kw)
    if L:
        return [("layers%d_r%d" % (k, r), dict(layers=k, reduce=r)) for k in (1, L) for r in (0, 1)] + [("area_layers%d" % L, dict(area=area, layers=L))]
    return [("plain", {}), ("reduce1", dict(reduce=1)), ("skip2", dict(skip_planes=2)), ("trunc_r0", dict(truncated=True)), ("trunc_r1", dict(truncated=True, reduce=1)),
            ("area", dict(area=area)), ("area_trunc", dict(area=area, truncated=True)), ("area_r1_skip1", dict(area=area, reduce=1, skip_planes=1))]


def dev_encode(E, p, fmt, d_pix, sop, kw, image=None):
    def go():
        res = p.encode_frame_image(image, sop=sop, eph=sop) if image is not None else p.encode_frame_pixels(fmt, d_pix, sop=sop, eph=sop, **kw)
        p.frame_status()
        out, toffs = res[0], res[1].cpu().numpy()
        rest = list(res[2:])
        loffs = rest.pop(0).cpu().numpy() if nlayers_of(kw) else None
        ach = rest.pop(0).cpu().numpy() if rest else None
        data = out[:int(toffs[-1])].cpu().numpy()
        rec = dict(stream=sha(data), tile_offs=sha(toffs.astype(np.int64)), layer_offs=None if loffs is None else sha(loffs.astype(np.int64)),
                   achieved=None if ach is None else sha(ach.astype(np.float64)))
        return rec, data
    r = E.run(go)
    if isinstance(r, dict):
        try:
            p.frame_status()                    # (a refused call leaves no status behind; a refused stream's was read above)
        except E.J2KError:
            pass
        return r, None
    return r


def host_encode(E, p, fmt, pix, sop, kw, image=None):
    def go():
        d = p.encode_image_host(image, sop=sop, eph=sop) if image is not None else p.encode_pixels_host(fmt, pix, sop=sop, eph=sop, **kw)
        rec = dict(stream=sha(d["bytes"]), tile_offs=sha(d["tile_offs"].astype(np.int64)), layer_offs=sha(d["layer_offs"].astype(np.int64)) if "layer_offs" in d else None,
                   achieved=sha(d["achieved"].astype(np.float64)) if "achieved" in d else None, lens=sha(d["lens"]), numbps=sha(d["numbps"]))
        return rec, d
    r = E.run(go)
    return (r, None) if isinstance(r, dict) else r


def decode_both(E, p, name, key, data, sop, combos):
    """`data` (numpy uint8, one stream) through the device method and the host method, for every combination"""
    torch = E.torch
    W, H, Cn, prec, fmt = PLANS[name][:5]
    bpp = 4 if fmt == RGBA8 else 2
    cs = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(p.device)
    for cid, kw in combos:
        red = int(kw.get("reduce", 0))
        def shape():
            if "area" in kw:
                h, w = p.area_shape(kw["area"], red)
                return (h, w * bpp)
            return ((H + (1 << red) - 1) >> red, W * bpp)
        def dev():
            back = torch.zeros(shape(), dtype=torch.uint8, device=p.device)
            p.decode_frame_pixels(cs, int(data.size), back, sop=sop, eph=sop, **kw)
            p.frame_status()
            return sha(back.cpu().numpy())
        r = E.run(dev)
        if isinstance(r, dict):
            try:
                p.frame_status()
            except E.J2KError:
                pass
        E.out["%s/%s/dev" % (key, cid)] = r
        E.out["%s/%s/host" % (key, cid)] = E.run(lambda: sha(p.decode_pixels_host(data, shape(), sop=sop, eph=sop, **kw)))


def collect_forms(E):
    torch = E.torch
    streams = {}                                  # plan name -> its plain stream without markers (the refusal table decodes it)
    for name in PLANS:
        W, H, Cn, prec, fmt = PLANS[name][:5]
        p = E.plan(name)
        try:
            pix = make_pixels(fmt, W, H, 1000 + ord(name))
            d_pix = torch.from_numpy(pix).to(p.device)
            plain = p.encode_pixels_host(fmt, pix)
            body = int(plain["lens"].astype(np.int64).sum())
            streams[name] = plain["bytes"]
            forms = [(fid, kw, None, None) for fid, kw in encode_forms(name, body)]
            if name in "AE":
                forms.append(("ycbcr420", {}, make_ycbcr(W, H, 77), make_ycbcr(W, H, 77, lambda a: torch.from_numpy(a).to(p.device))))
            for fid, kw, h_img, d_img in forms:
                for sop in (False, True):
                    key = "%s/%s/se%d" % (name, fid, int(sop))
                    rd, data_d = dev_encode(E, p, fmt, d_pix, sop, kw, d_img)
                    rh, dh = host_encode(E, p, fmt, pix, sop, kw, h_img)
                    E.out[key + "/enc/dev"], E.out[key + "/enc/host"] = rd, rh
                    if fid == "layers3" and not sop and dh is not None:
                        streams[name + "/layers3"] = dh["bytes"]
                    combos = decode_combos(name, kw)
                    if data_d is not None:
                        decode_both(E, p, name, key + "/dec", data_d, sop, combos)
                    if dh is not None and (data_d is None or not np.array_equal(dh["bytes"], data_d)):
                        decode_both(E, p, name, key + "/dec_hoststream", dh["bytes"], sop, combos)
        finally:
            p.close()
    return streams


# ---- refusals: every frame entry point through ctypes, a table of bad calls ------------------------------------------------------------------------
ENC = "P fmt pix stride sop eph"
ENTRIES = {        # name -> (host form?, parameter names in order)
    "j2k_plan_encode_frame_pixels": (0, ENC + " out cap toffs"),
    "j2k_plan_encode_frame_pixels_rate": (0, ENC + " budget out cap toffs"),
    "j2k_plan_encode_frame_pixels_layers": (0, ENC + " budgets nl out cap toffs loffs"),
    "j2k_plan_encode_frame_pixels_roi": (0, ENC + " budgets nl roi gain out cap toffs loffs"),
    "j2k_plan_encode_frame_pixels_quality": (0, ENC + " targets nl roi gain out cap toffs loffs ach"),
    "j2k_plan_encode_frame_image": (0, "P img sop eph out cap toffs"),
    "j2k_encode_pixels_host": (1, ENC + " out cap olen toffs lens nbps"),
    "j2k_encode_pixels_host_rate": (1, ENC + " budget out cap olen toffs lens nbps"),
    "j2k_encode_pixels_host_layers": (1, ENC + " budgets nl out cap olen toffs loffs lens nbps"),
    "j2k_encode_pixels_host_roi": (1, ENC + " budgets nl roi gain out cap olen toffs loffs lens nbps"),
    "j2k_encode_pixels_host_quality": (1, ENC + " targets nl roi gain out cap olen toffs loffs lens nbps ach"),
    "j2k_encode_image_host": (1, "P img sop eph out cap olen toffs lens nbps"),
    "j2k_plan_decode_frame_pixels": (0, "P cs len in_toffs sop eph dst dstride"),
    "j2k_plan_decode_frame_pixels_reduced": (0, "P cs len in_toffs sop eph reduce dst dstride"),
    "j2k_plan_decode_frame_pixels_coarse": (0, "P cs len in_toffs sop eph reduce skip dst dstride"),
    "j2k_plan_decode_frame_pixels_rate": (0, "P cs len in_toffs sop eph reduce skip dst dstride"),
    "j2k_plan_decode_frame_pixels_layers": (0, "P cs len in_toffs sop eph layers reduce skip dst dstride"),
    "j2k_plan_decode_frame_pixels_area": (0, "P cs len in_toffs sop eph layers truncated reduce skip area dst dstride"),
    "j2k_decode_pixels_host": (1, "P cs len sop eph dst dstride"),
    "j2k_decode_pixels_host_reduced": (1, "P cs len sop eph reduce dst dstride"),
    "j2k_decode_pixels_host_coarse": (1, "P cs len sop eph reduce skip dst dstride"),
    "j2k_decode_pixels_host_rate": (1, "P cs len sop eph reduce skip dst dstride"),
    "j2k_decode_pixels_host_layers": (1, "P cs len sop eph layers reduce skip dst dstride"),
    "j2k_decode_pixels_host_area": (1, "P cs len sop eph layers truncated reduce skip area dst dstride"),
}
I64 = lambda *v: (C.c_int64 * len(v))(*v)
F64 = lambda *v: (C.c_double * len(v))(*v)
BAD_W = 97          # a rectangle one column outside every plan's frame but B's, where it is 17 outside
# (label, plan, overrides, only the entries whose name contains this); an override applies where the entry has that parameter, and a row
# applies to an entry that has at least one of its parameters (a row without overrides: to every entry)
ROWS = [
    ("ht", "C", {}, ""),
    ("ht_negative_budget", "C", dict(budget=-1, budgets=I64(-1), nl=1, targets=F64(-1.0)), "encode"),
    ("ht_skip1", "C", dict(skip=1), ""),
    ("prefix_plan", "D", {}, ""),
    ("prefix_inverted_rect", "D", dict(roi=(90, 11, 37, 40), area=(90, 11, 37, 40)), ""),
    ("not_closed_loop", "E", {}, ""),
    ("raw_magref", "F", {}, ""),
    ("raw_magref_truncated", "F", dict(truncated=1), ""),
    ("raw_magref_layers2", "F", dict(layers=2), ""),
    ("null_plan", "A", dict(P=None), ""),
    ("null_plan_null_out", "A", dict(P=None, out=None, dst=None), ""),
    ("ht_null_out", "C", dict(out=None, dst=None), ""),
    ("prefix_null_out", "D", dict(out=None, dst=None), ""),
    ("not_closed_loop_null_out", "E", dict(out=None, dst=None), ""),
    ("null_out", "A", dict(out=None, dst=None), ""),
    ("null_toffs", "A", dict(toffs=None), "j2k_plan_encode"),
    ("null_pix", "A", dict(pix=None, cs=None, img=None), ""),
    ("null_olen", "A", dict(olen=None), ""),
    ("negative_budget", "A", dict(budget=-1, budgets=I64(-1), nl=1, targets=F64(-1.0)), ""),
    ("negative_budget_null_out", "A", dict(budget=-1, budgets=I64(-1), nl=1, targets=F64(-1.0), out=None), ""),
    ("no_budgets", "A", dict(budgets=None, targets=None), ""),
    ("no_budgets_bad_gain", "A", dict(budgets=None, targets=None, gain=0), ""),
    ("nl0", "A", dict(nl=0), ""),
    ("nl33", "A", dict(nl=33, budgets=I64(*([1000] * 33)), targets=F64(*([1e6] * 33))), ""),
    ("nl0_roi_outside", "A", dict(nl=0, roi=(0, 0, BAD_W, 4)), ""),
    ("nl2_no_layer_offs", "A", dict(nl=2, budgets=I64(500, 1000), targets=F64(2e6, 1e6), loffs=None), ""),
    ("nl2_no_layer_offs_roi_outside", "A", dict(nl=2, budgets=I64(500, 1000), targets=F64(2e6, 1e6), loffs=None, roi=(0, 0, BAD_W, 4)), ""),
    ("rising_targets", "A", dict(nl=2, targets=F64(1e6, 2e6)), ""),
    ("falling_budgets", "A", dict(nl=2, budgets=I64(1000, 999)), ""),
    ("falling_budgets_inverted_roi", "A", dict(nl=2, budgets=I64(1000, 999), targets=F64(1e6, 2e6), roi=(90, 11, 37, 40)), ""),
    ("bad_gain", "A", dict(gain=65536), ""),
    ("bad_gain_null_roi", "A", dict(gain=0, roi=None), ""),
    ("null_roi", "A", dict(roi=None, area=None), ""),
    ("bad_format", "A", dict(fmt=99), ""),
    ("bad_format_negative_budget", "A", dict(fmt=99, budget=-1, budgets=I64(-1), nl=1, targets=F64(-1.0)), ""),
    ("layers0", "A", dict(layers=0), ""),
    ("layers33", "A", dict(layers=33), ""),
    ("layers33_skip32", "A", dict(layers=33, skip=32), ""),
    ("layers0_reduce_beyond", "A", dict(layers=0, reduce=5), ""),
    ("skip32", "A", dict(skip=32), ""),
    ("skip_negative", "A", dict(skip=-1), ""),
    ("skip32_null_dst", "A", dict(skip=32, dst=None), ""),
    ("reduce_beyond", "A", dict(reduce=5), ""),
    ("reduce_negative", "A", dict(reduce=-1), ""),
    ("reduce_beyond_null_dst", "A", dict(reduce=5, dst=None), ""),
    ("reduce_beyond_skip32", "A", dict(reduce=5, skip=32), ""),
    ("area_outside", "A", dict(area=(0, 0, BAD_W, 4)), ""),
    ("area_outside_skip32", "A", dict(area=(0, 0, BAD_W, 4), skip=32), ""),
    ("area_outside_layers33", "A", dict(area=(0, 0, BAD_W, 4), layers=33), ""),
    ("area_small_stride", "A", dict(dstride=8), "_area"),
    ("area_small_stride_null_dst", "A", dict(dstride=8, dst=None), "_area"),
    ("area_layers33_small_stride", "A", dict(dstride=8, layers=33), "_area"),
    ("gray_lossy_layers33", "B", dict(layers=33, nl=33), ""),
    ("gray_lossy_rgba_format", "B", dict(fmt=RGBA8), "encode"),
    ("small_cap", "A", dict(cap=16), "encode"),
]


class Caller:
    """valid arguments of every frame entry point for one plan; call(name, **overrides) -> [status, frame status after it]"""

    def __init__(self, E, name, p, streams):
        torch = E.torch
        cs, layered = streams[name], streams.get(name + "/layers3", streams[name])      # (the _layers decodes read a layered stream where the plan writes one)
        self.E, self.p = E, p
        W, H, Cn, prec, fmt = PLANS[name][:5]
        bpp = 4 if fmt == RGBA8 else 2
        n, nt = int(p.info.blocks), int(p.info.tiles)
        pix = make_pixels(fmt, W, H, 5)
        aw = PLANS[name][7][2] - PLANS[name][7][0]
        cap = 1 << 18
        dev = lambda k, dt=torch.uint8: torch.zeros(max(int(k), 8), dtype=dt, device=p.device)
        self.keep = dict(pix=(torch.from_numpy(pix).to(p.device), pix), out=(dev(cap), np.zeros(cap, np.uint8)), toffs=(dev(nt + 1, torch.int64), np.zeros(nt + 1, np.uint64)),
                         loffs=(dev(nt * 33, torch.int64), np.zeros(nt * 33, np.uint64)), ach=(dev(33, torch.float64), np.zeros(33, np.float64)),
                         cs=(torch.from_numpy(np.concatenate([cs, np.zeros(64, np.uint8)])).to(p.device), np.concatenate([cs, np.zeros(64, np.uint8)])),
                         lcs=(torch.from_numpy(np.concatenate([layered, np.zeros(64, np.uint8)])).to(p.device), np.concatenate([layered, np.zeros(64, np.uint8)])),
                         dst=(dev(H * W * bpp), np.zeros(H * W * bpp, np.uint8)),
                         img=(make_ycbcr(W, H, 6, lambda a: torch.from_numpy(a).to(p.device)), make_ycbcr(W, H, 6)))
        self.lens, self.nbps, self.olen = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8), C.c_size_t(0)
        self.base = dict(P=p.h, fmt=fmt, stride=W * bpp, sop=0, eph=0, cap=cap, budget=4000, budgets=I64(1000, 2000, 3000), nl=3, targets=F64(3e6, 2e6, 1e6),
                         roi=PLANS[name][6], gain=16, len=int(cs.size), in_toffs=None, reduce=0, skip=0, layers=0, truncated=0, area=PLANS[name][7],
                         dstride=W * bpp, lens="lens", nbps="nbps", olen="olen")
        self.area_stride, self.layered_len = aw * bpp, int(layered.size)

    def arg(self, k, v, host):
        lib = self.E.lib
        if k in self.keep and isinstance(v, str):                   # "buf": the valid buffer of that name
            a = self.keep[v if v != "buf" else k][host]
            if k == "img":
                self.img_struct = a.struct()
                return C.byref(self.img_struct)
            return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(C.c_void_p)
        if k in ("roi", "area"):
            if v is None:
                return None
            self.rects = getattr(self, "rects", []) + [lib.Rect(*v)]
            return C.byref(self.rects[-1])
        if k == "lens":
            return self.lens.ctypes.data_as(C.c_void_p)
        if k == "nbps":
            return self.nbps.ctypes.data_as(C.c_void_p)
        if k == "olen":
            return C.byref(self.olen) if v is not None else None
        if k in ("stride", "cap", "len", "dstride"):
            return C.c_size_t(int(v))
        if k == "budget":
            return C.c_int64(int(v))
        return v

    def call(self, entry, over, after=True):
        host, names = ENTRIES[entry]
        names = names.split()
        vals = dict(self.base)
        for k in self.keep:
            vals[k] = "buf"
        if entry.endswith("_area"):
            vals["dstride"] = self.area_stride
        if entry.endswith("_layers") and "decode" in entry:
            vals.update(cs="lcs", len=self.layered_len, layers=2)
        vals.update({k: v for k, v in over.items() if k in names})
        st = int(getattr(self.E.L, entry)(*[self.arg(k, vals[k], host) for k in names]))
        if not after:
            return st
        return [st, int(self.E.L.j2k_plan_frame_status(self.p.h))]   # (synchronises; reads and resets the status word)


def collect_refusals(E, streams):
    plans = {}
    try:
        for label, name, over, only in ROWS:
            if name not in plans:
                p = E.plan(name)
                plans[name] = (p, Caller(E, name, p, streams))
            for entry, (host, names) in ENTRIES.items():
                names = names.split()
                if only not in entry or (over and not any(k in names for k in over if k != "P") and "P" not in over):
                    continue
                E.out["refuse/%s/%s" % (label, entry)] = plans[name][1].call(entry, over)
        # the area host decode reads the frame status before it copies back: a refused stream (a corrupted SOT) leaves pix as it was
        p, cl = plans["A"]
        bad = streams["A"].copy()
        bad[0:2] = 0
        pix = np.full((PLANS["A"][7][3] - PLANS["A"][7][1], cl.area_stride), FILL, np.uint8)
        r = E.run(lambda: p.decode_pixels_host(bad, pix.shape, area=PLANS["A"][7], pix=pix))
        E.out["refuse/area_host_corrupt_sot"] = [r if isinstance(r, dict) else "decoded", bool((pix == FILL).all())]
        r = E.run(lambda: p.decode_pixels_host(bad, (PLANS["A"][1], PLANS["A"][0] * 4)) is not None)
        E.out["refuse/host_corrupt_sot"] = r if isinstance(r, dict) else "decoded"
    finally:
        for p, _ in plans.values():
            p.close()


# ---- capture: one encode form and one decode form, one warm call, captured once, replayed on a second input -----------------------------------------
def collect_capture(E, streams):
    torch, lib = E.torch, E.lib
    from j2kgfx import Context
    W, H, Cn, prec, fmt = PLANS["A"][:5]
    roi = lib.Rect(*PLANS["A"][6])
    ctx = Context(0)
    p = E.plan("A", ctx)
    try:
        L, nt = ctx.L, int(p.info.tiles)
        frames = [torch.from_numpy(make_pixels(fmt, W, H, s)).to(p.device) for s in (31, 32)]
        d_pix = frames[0].clone()
        body = int(p.encode_pixels_host(fmt, frames[0].cpu().numpy())["lens"].astype(np.int64).sum())
        budgets = I64(body // 4, body // 2)
        out = torch.zeros(p.frame_bound_layers(2), dtype=torch.uint8, device=p.device)
        toffs, loffs = torch.zeros(nt + 1, dtype=torch.int64, device=p.device), torch.zeros(2 * nt, dtype=torch.int64, device=p.device)
        back = torch.zeros(((H + 1) // 2, W * 4), dtype=torch.uint8, device=p.device)
        enc = lambda: L.j2k_plan_encode_frame_pixels_roi(p.h, fmt, C.c_void_p(d_pix.data_ptr()), C.c_size_t(W * 4), 1, 1, budgets, 2, C.byref(roi), 16, C.c_void_p(out.data_ptr()),
                                                         C.c_size_t(int(out.numel())), C.c_void_p(toffs.data_ptr()), C.c_void_p(loffs.data_ptr()))
        dec = lambda: L.j2k_plan_decode_frame_pixels_layers(p.h, C.c_void_p(out.data_ptr()), C.c_size_t(int(out.numel())), C.c_void_p(toffs.data_ptr()), 1, 1, 2, 1, 0,
                                                            C.c_void_p(back.data_ptr()), C.c_size_t(W * 4))
        torch.cuda.synchronize()
        E.out["capture/warm"] = [int(enc()), int(dec()), int(L.j2k_plan_frame_status(p.h))]
        cl = Caller(E, "A", p, streams)
        with ctx.capture() as g:
            E.out["capture/calls"] = [int(enc()), int(dec())]
            for entry, (host, names) in ENTRIES.items():            # every host call refuses while the context captures
                if host:
                    E.out["refuse/capturing/%s" % entry] = cl.call(entry, {}, after=False)
        for i in (1, 0):
            d_pix.copy_(frames[i])
            out.zero_()
            back.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            st = int(L.j2k_plan_frame_status(p.h))
            t = toffs.cpu().numpy()
            E.out["capture/replay%d" % i] = dict(status=st, stream=sha(out[:int(t[-1])].cpu().numpy()), tile_offs=sha(t), layer_offs=sha(loffs.cpu().numpy()),
                                                 pixels=sha(back.cpu().numpy()))
        g.close()
    finally:
        p.close()
        ctx.close()


def collect():
    E = Env()
    try:
        streams = collect_forms(E)
        collect_refusals(E, streams)
        collect_capture(E, streams)
        return E.out
    finally:
        E.close()


# ---- the test ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def got():
    return collect()


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


def test_same_cases(got, recorded):
    assert sorted(got) == sorted(recorded)


@pytest.mark.parametrize("group", ["A/", "B/", "C/", "D/", "E/", "F/", "refuse/", "capture/"])
def test_as_recorded(got, recorded, group):
    """every recorded case of the group is asserted: the value the calls give now is the value they gave when the JSON was written"""
    want = {k: v for k, v in recorded.items() if k.startswith(group)}
    assert want, group
    have = json.loads(json.dumps({k: got.get(k) for k in want}))
    differ = {k: (have[k], want[k]) for k in want if have[k] != want[k]}
    assert not differ, "%d of %d cases differ: %s" % (len(differ), len(want), dict(list(differ.items())[:8]))


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "go-jpeg2000_amd")):
        sys.path.insert(0, d)
    os.environ.setdefault("J2K_TUNING", "1")
    res = collect()
    with open(sys.argv[1] if len(sys.argv) > 1 else RECORDED, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases recorded" % len(res))
