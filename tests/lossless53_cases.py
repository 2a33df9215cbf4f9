"""Named, seeded cases for the lossless 5-3 path (csrc/dwt53.hip, dwt53_deep.inc, dwt53_plane_wg.inc, dwt53_l0pix.inc,
dwt53_l0pix_fwd_body.inc): the shapes at which its kernel forms change behaviour and the contents that make a mistake visible where it
happens.  Importable without a GPU: tests/test_lossless53_cases.py checks the lists on the CPU, tests/test_gpu_lossless53_oracle.py runs
them against the C oracle on the device.  This is the place to add a shape when a 5-3 kernel form changes.

Constants come from the code: the context defaults from csrc/j2k_plan.h (defaults()), the values every option accepts from the
ctx_options() table of csrc/j2k_ctx.cpp (option_values()).  route() restates the plan builder (csrc/j2k_planbuild.cpp) and the packed-pixel
admission rule (pix_fusable, csrc/j2k_stages.cpp) in plain Python: tile grid, per-level planes, pick_cpl, the vec_ok rule, make_jobs' strips
and bands, the link rule, the workgroup forms' admission, tail / deep / mega / fused conditions.  It is used ONLY to choose and label
cases (forms()) and to put edges on seams (seams()); no test compares a device result with it.

Contents: `noise` is what the older tests use; `fullrange` spans int32 (Go's arithmetic wraps); `impulse` and `step` put an edge on every
strip seam column, band seam row, link seam, the last row and the last column of the case's own job tables; `const` is 0 in one half of the
components and 2^prec - 1 in the other; `checker` is the largest high-pass signal.  Coefficient sets for the inverse come from no forward
transform: `noise`, `fullrange`, `impulse`, and `pixelrange` -- reconstructions that leave 0 ... 2^prec - 1 on a few rows and stay inside
it on the others, searched for with the oracle."""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-jpeg2000_amd", "csrc")
PLAN_H = os.path.join(CSRC, "j2k_plan.h")
CTX_CPP = os.path.join(CSRC, "j2k_ctx.cpp")

DEFAULT_NAMES = ("band_prows", "band_prows_pix", "plane_wg", "l0_wg", "l0_wg_invw", "deep_min_planes")
# the other fields of the context the routing reads (option name -> field where they differ)
OTHER_FIELDS = ("band_prows_inv", "fwd_link", "inv_link", "pix_fuse", "plane_wg3", "l0_fuse", "l0_inv_wpe", "l0_wg_inv", "l0_store", "use_tail",
                "use_deep", "deep_mid", "deep_mid_inv", "mega", "xcd_map", "cpl0", "force_novec", "fwd_pf")
OPTION_FIELD = {"deep": "use_deep"}
OPTIONS_53 = ("plane_wg", "l0_wg", "l0_wg_invw", "l0_fuse", "l0_inv_wpe", "l0_store", "deep", "deep_mid", "deep_mid_inv", "mega", "plane_wg3",
              "pix_fuse", "l0_wg_inv")
PRECISIONS = (8, 12, 16, 31)
NRES = (1, 2, 3, 4, 6, 0)            # 0: none given, the reference's five levels (encoder.go:249-252); 1 is five levels too (levels <= 0)
FRAME_FAMILIES = ("noise", "fullrange", "impulse", "step", "const", "checker")
COEFF_FAMILIES = ("noise", "fullrange", "impulse")
PIXELRANGE_MIN_H = 6                 # below this no tile has two rows out of reach of a level-0 high-pass row
PIX_NAMES = ("gray8", "gray16", "rgba8", "rgba64", "nrgba8", "nrgba64")
PIX_COMP = (1, 1, 3, 3, 4, 4)
PIX_BPS = (1, 2, 1, 2, 1, 2)
PIX_BYTES = (1, 2, 4, 8, 4, 8)
LINK_DOWN, LINK_UP = 1, 2


def _field(text, name):
    m = re.search(r"\b(?:int|bool|long)\s+%s\s*=\s*(-?\w+)\s*;" % name, text)
    assert m, "no default for %s in %s" % (name, PLAN_H)
    return {"true": 1, "false": 0}[m.group(1)] if m.group(1) in ("true", "false") else int(m.group(1))


@functools.lru_cache(None)
def defaults():
    """{band_prows, band_prows_pix, plane_wg, l0_wg, l0_wg_invw, deep_min_planes}: the context defaults, from the struct that holds them"""
    with open(PLAN_H) as f:
        text = f.read()
    return {n: _field(text, n) for n in DEFAULT_NAMES}


@functools.lru_cache(None)
def all_defaults():
    with open(PLAN_H) as f:
        text = f.read()
    return {n: _field(text, n) for n in DEFAULT_NAMES + OTHER_FIELDS}


@functools.lru_cache(None)
def option_values():
    """{option: the values j2k_ctx_set_option accepts (0 ... 32)} from the OPT(name, condition, ...) lines of ctx_options()"""
    with open(CTX_CPP) as f:
        text = f.read()
    out = {}
    for name, cond in re.findall(r'OPT\("(\w+)",\s*(.+?),\s*c->', text):
        expr = cond.replace("||", " or ").replace("&&", " and ")
        out[name] = tuple(v for v in range(0, 33) if eval(expr, {"__builtins__": {}}, {"v": v}))
    return out


def options(env=()):
    """the context a set of J2K_* variables gives: every value must be one the option table accepts"""
    o = dict(all_defaults())
    for k, v in dict(env).items():
        name = k[4:].lower()
        if name == "deep_min_planes":
            o[name] = int(v)
            continue
        assert int(v) in option_values()[name], (k, v)
        o[OPTION_FIELD.get(name, name)] = int(v)
    return o


def levels_of(nres):
    return nres - 1 if nres - 1 > 0 else 5          # encoder.go:249-252


def tiles_of(W, H, tile):
    """(x0, y0, w, h) of every tile, in the plan's order"""
    tw, th = tile[0] or W, tile[1] or H
    return [(x0, y0, min(tw, W - x0), min(th, H - y0)) for y0 in range(0, H, th) for x0 in range(0, W, tw)]


def at_level(w, h, l):
    for _ in range(l):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


# ---- the plan builder, restated ---------------------------------------------------------------------------------------------------------
def pick_cpl(maxw):
    return 8 if maxw >= 384 else (4 if maxw >= 192 else 2)


def lds_fits(w, h):
    return w <= 128 and w * h <= 16384


def make_jobs(plane, w, h, cpl, band):
    """[plane, col0, prow0, nprow, link]: strips of 64 lanes of cpl columns that advance by 63 lanes (one halo lane on either side), bands of
    `band` pair-rows"""
    half, col0, out = (h + 1) // 2, 0, []
    while True:
        c_base = col0 - (cpl if col0 else 0)
        out += [[plane, col0, pr, band, 0] for pr in range(0, max(half, 1), band)]
        if c_base + 64 * cpl >= w:
            return out
        col0 = c_base + 63 * cpl


def link_jobs(jobs, dims):
    """vertically adjacent bands that share a workgroup (four consecutive jobs) exchange halo rows through LDS"""
    for i in range(1, len(jobs)):
        if i % 4 == 0:
            continue
        a, b = jobs[i - 1], jobs[i]
        if a[0] != b[0] or a[1] != b[1]:
            continue
        w, h = dims[a[0]]
        half = (h + 1) // 2
        if w < 2 or h < 2 or a[2] + a[3] != b[2]:
            continue
        if min(a[3], half - a[2]) < 2 or min(b[3], half - b[2]) < 2 or 2 * b[2] + 1 >= h:
            continue
        a[4] |= LINK_DOWN
        b[4] |= LINK_UP
    return jobs


Tab = collections.namedtuple("Tab", "level cls planes cpl vec jobs pwg")       # planes: (x0, y0, w, h) with the tile's origin in the frame


def route(W, H, C, tile, nres, env=()):
    """what build_plan makes of a lossless frame: a dict with the per-level tables (key (level, cls); both directions share them while
    band_prows_inv is 0), tail_l0, deep_l0, the deep launch's planes, the RGBA8 level-0 tables and how many per-level launches run"""
    o = options(env)
    assert o["band_prows_inv"] == 0 and o["fwd_link"] == o["inv_link"] == 1 and not o["xcd_map"] and not o["cpl0"] and not o["force_novec"]
    L = levels_of(nres)
    triple = C >= 3
    groups = []                                   # (x0, y0, w, h, comp0, nc)
    for x0, y0, w, h in tiles_of(W, H, tile):
        c = 0
        while c < C:
            nc = 3 if (triple and c == 0) else 1
            groups.append((x0, y0, w, h, c, nc))
            c += nc
    R = dict(W=W, H=H, C=C, L=L, opts=o, groups=groups, tail_l0=-1, deep_l0=-1, deep=[], tabs={}, rgba8={})
    if o["use_tail"] and L >= 3:
        for l0 in range(1, L - 1):
            if all(lds_fits(*at_level(g[2], g[3], l0)) for g in groups):
                R["tail_l0"] = l0
                break
    lds_l0 = -1
    for l0 in range(1, L):
        if all(lds_fits(*at_level(g[2], g[3], l0)) for g in groups):
            lds_l0 = l0
            break
    if lds_l0 >= 2 and o["use_deep"]:
        l0, ok, planes = lds_l0 - 1, True, []
        for g in groups:
            w, h = at_level(g[2], g[3], l0)
            if w < 8 or w > 256 or w % 4 or h < 2 or h > 256:
                ok = False
                break
            w1, h1 = w // 2, (h + 1) // 2
            w2, h2 = (w1 + 1) // 2, (h1 + 1) // 2
            if w1 > 128 or w1 * h1 > 16384:
                ok = False
                break
            T = (h1 + 1) // 2
            T1 = (T + 1) // 2
            has_mid = bool(o["deep_mid"] and T >= 2 and w % 8 == 0 and w1 % 2 == 0 and 64 % (w1 // 2) == 0 and h1 >= 2)
            nn1 = w2 * h2 if L - l0 > 2 else 0
            compact = has_mid and o["deep_mid_inv"] == 1 and w1 % 4 == 0 and nn1 % 4 == 0
            mid_inv = o["deep_mid_inv"] if has_mid else 0
            for _ in range(g[5]):
                planes.append(dict(x0=g[0], y0=g[1], w=w, h=h, T=T, T1=T1, has_mid=has_mid, compact=compact, mid_inv=mid_inv, nlev=L - l0,
                                   flat=list(range(T, h1, 64)), half=h1))
        if ok and len(planes) < o["deep_min_planes"]:
            ok = False
        if ok and planes:
            R["deep_l0"], R["deep"] = l0, planes
    R["nlaunch"] = R["deep_l0"] if R["deep_l0"] >= 0 else (R["tail_l0"] if R["tail_l0"] >= 0 else L)
    for l in range(L):
        for cls in (0, 1):
            planes, dims, offs = [], [], []
            for x0, y0, w, h, c0, nc in groups:
                as_triple = nc == 3 and l == 0
                if (cls == 1) != as_triple:
                    continue
                lw, lh = at_level(w, h, l)
                for k0 in range(1 if as_triple else nc):
                    planes.append((x0, y0, lw, lh))
                    dims.append((lw, lh))
                    ks = range(3) if as_triple else (k0,)
                    offs.append([(c0 + k) * H * W + y0 * W + x0 for k in ks] if l == 0 else [0])
            if not planes:
                continue
            maxw = max(w for w, _ in dims)
            cpl = pick_cpl(maxw)
            vec = all(w % cpl == 0 for w, _ in dims) and (l != 0 or W % cpl == 0) and all(f % 4 == 0 for fs in offs for f in fs)
            if not vec:
                cpl = 2
            jobs = []
            for i, (w, h) in enumerate(dims):
                jobs += make_jobs(i, w, h, cpl, o["band_prows"])
            link_jobs(jobs, dims)
            pwg = None
            if vec and o["plane_wg"] > 0 and (cls == 0 or o["plane_wg3"] or l == 0):
                ok = all(w >= 16 and w % 8 == 0 and h >= 2 for w, h in dims) and (l != 0 or W % 8 == 0)
                multi = any(w > 512 for w, _ in dims)
                if ok and maxw < 512 and sum((h + 1) // 2 for _, h in dims) > 4096:
                    ok = False
                if ok:
                    nr = o["plane_wg"] - 1
                    pj = [[i, c0, pr, nr, 0] for i, (w, h) in enumerate(dims) for c0 in range(0, w, 512) for pr in range(0, (h + 1) // 2, nr)]
                    pwg = dict(nw=o["plane_wg"], multi=multi, pix_only=(cls == 1 and not o["plane_wg3"]), jobs=pj)
            R["tabs"][(l, cls)] = Tab(l, cls, planes, cpl, vec, jobs, pwg)
            if l == 0 and cls == 1 and vec and cpl == 8:
                R["rgba8"] = _rgba8_tables(R, o, dims, L, len(planes) == len(groups))
    return R


def _split_row(h, nr):
    half = (h + 1) // 2
    tb = (half + 1) // 2
    return min(half, ((tb + nr - 1) // nr) * nr)


def _rgba8_tables(R, o, dims, L, only_triples):
    """the packed-pixel level-0 tables of the RGB triples: shorter marching bands, the workgroup forms of both directions, levels 0 + 1 in one
    launch, the merged launches"""
    pix = []
    for i, (w, h) in enumerate(dims):
        pix += make_jobs(i, w, h, 8, o["band_prows_pix"])
    link_jobs(pix, dims)
    out = dict(pix_jobs=pix, fwd_wg=None, inv_wg=None, fuse=None, mega=None)
    if not (o["l0_wg"] > 0 and all(16 <= w <= 512 and w % 8 == 0 and h >= 2 for w, h in dims)):
        return out

    def table(waves, top_only=False):
        nr = waves - 1
        return [[i, 0, pr, nr, 0] for i, (_, h) in enumerate(dims) for pr in range(0, _split_row(h, nr) if top_only else (h + 1) // 2, nr)]

    invw = o["l0_wg_invw"] or o["l0_wg"]
    out["fwd_wg"] = dict(nw=o["l0_wg"], jobs=table(o["l0_wg"]))
    out["inv_wg"] = dict(nw=invw, jobs=table(invw))
    if o["mega"] and R["deep_l0"] == 1 and R["C"] == 3 and only_triples and R["deep"]:
        m = dict(order=o["mega"])
        for d, waves in (("fwd", o["l0_wg"]), ("inv", invw)):
            m[d] = dict(top=table(waves, True),
                        bands=[[i, 2, pr, 15, 0] for i, (_, h) in enumerate(dims) for pr in range(_split_row(h, waves - 1), (h + 1) // 2, 15)])
        out["mega"] = m
    if o["l0_fuse"] > 0 and L >= 2 and R["C"] == 3 and (R["tail_l0"] < 0 or R["tail_l0"] >= 2) and (R["deep_l0"] < 0 or R["deep_l0"] >= 2):
        nr2, nr, fj, rj = o["l0_fuse"] - 3, o["l0_wg"] - 1, [], []
        for i, (_, h) in enumerate(dims):
            half = (h + 1) // 2
            half1 = (half + 1) // 2
            pr = 0
            while pr < half1:
                fj.append([i, 0, pr, nr2, 0])
                pr += nr2
            while pr < half:
                rj.append([i, 0, pr, nr, 0])
                pr += nr
        out["fuse"] = dict(nw=o["l0_fuse"], top=fj, rest=rj)
    return out


def pix_fusable(R, fmt_bps, channels, stride, inverse, prec):
    """pix_fusable (csrc/j2k_stages.cpp), 5-3 branch: None when the frame is staged through int32 planes, else (single, triple): what the
    single planes read / write (SRC / DST 1 ... 4; 0 = none) and what the triples do (8 = the RGBA8 kernels, 4 = RGBA64 through the plane
    kernels)"""
    o, W, C = R["opts"], R["W"], R["C"]
    pb = fmt_bps * channels
    if R["L"] < 1 or prec != 8 * fmt_bps or W % 8:
        return None
    if o["pix_fuse"] == 0 or (o["pix_fuse"] == 2 and not (fmt_bps == 1 and channels == 4 and C == 3) and not (fmt_bps == 2 and channels == 1)):
        return None
    if stride % 16 or stride < W * pb:
        return None
    T0, T1 = R["tabs"].get((0, 0)), R["tabs"].get((0, 1))
    if not T0 and not T1:
        return None
    single = triple = 0
    if T0:
        single = (1 if fmt_bps == 2 else 2) if channels == 1 else (4 if fmt_bps == 2 else 3)
        wg = T0.pwg is not None
        if single == 1:
            if not (wg or (T0.vec and T0.cpl == 8)) or T1:
                return None
        elif not (wg and T0.pwg["nw"] == 4):
            return None
    if T1:
        if channels != 4 or C < 3:
            return None
        if fmt_bps == 1:
            if not T1.vec or T1.cpl != 8:
                return None
            triple = 8
        else:
            if not T1.pwg or T1.pwg["nw"] != 4:
                return None
            triple = 4
    if inverse and channels == 4 and not T1 and C != 4:
        return None
    if inverse and channels == 4 and T0 and not (T1 and C - 3 <= 1):
        return None
    return single, triple


def forms(R, direction, entry="frame", fmt=None, stride=None, prec=None):
    """the kernel forms one call runs, as labels: entry `frame` (j2k_plan_forward / _inverse on an int32 frame), `unit` (the host calls: the same
    tables on a cached one-component plan) or `pixels` (j2k_plan_forward_pixels / _inverse_pixels / _rgba8 on format `fmt`).  A route is
    (label, direction, `i32` / `unit` / the format's name)."""
    o = R["opts"]
    fused = None
    io = "unit" if entry == "unit" else "i32"
    pio = PIX_NAMES[fmt] if entry == "pixels" else io          # only a kernel that reads / writes the pixels itself is a packed route
    if entry == "pixels":
        fused = pix_fusable(R, PIX_BPS[fmt], 1 if R["C"] == 1 else 4, stride, direction == "inv", prec)
    out = set()
    for (l, cls), T in R["tabs"].items():
        if l >= R["nlaunch"]:
            continue
        nc = 3 if cls else 1
        src = 0
        if l == 0 and fused:
            single, triple = fused
            src = (4 if triple == 4 else 0) if cls else single
            if cls and triple == 8:
                r8 = R["rgba8"]
                if direction == "fwd":
                    if r8["fwd_wg"]:
                        if r8["fuse"]:
                            out.add(("rgba8_fuse<nw%d,store%d>" % (r8["fuse"]["nw"], 0 if o["l0_store"] == 0 else 1), pio))
                            if r8["fuse"]["rest"]:
                                out.add(("rgba8_wg_fwd<nw%d,store%d>" % (r8["fwd_wg"]["nw"], o["l0_store"]), pio))
                        else:
                            out.add(("rgba8_wg_fwd<nw%d,store%d>" % (r8["fwd_wg"]["nw"], o["l0_store"]), pio))
                    else:
                        out.add(("march<cpl8,nc3,vec,pix>", pio))
                else:
                    if r8["inv_wg"] and o["l0_wg_inv"]:
                        out.add(("rgba8_wg_inv<nw%d,wpe%d>" % (r8["inv_wg"]["nw"], o["l0_inv_wpe"]), pio))
                    else:
                        out.add(("march<cpl8,nc3,vec,pix>", pio))
                continue
        pwg = T.pwg if (T.pwg and (not T.pwg["pix_only"] or src == 4)) else None
        if pwg and (nc == 1 or src in (0, 4)):
            out.add(("plane_wg<nw%d,nc%d,io%d,%s>" % (pwg["nw"], nc, src, "multi" if pwg["multi"] else "single"), pio if src else io))
        else:
            out.add(("march<cpl%d,nc%d,%s%s>" % (T.cpl, nc, "vec" if T.vec else "scalar", ",pix" if src else ""), pio if src else io))
    r8 = R["rgba8"]
    mega = bool(entry == "pixels" and fused and fused[1] == 8 and r8.get("mega") and r8["fwd_wg"]
                and (not r8["fuse"] if direction == "fwd" else o["l0_wg_inv"]))      # (the fused forward launch takes precedence over the merged one)
    if R["deep_l0"] >= 0:
        for p in R["deep"]:
            tag, dio = ("mega_", pio) if mega else ("", io)
            if mega:
                out.add(("mega_%s<order%d>" % (direction, r8["mega"]["order"]), pio))
            if direction == "fwd":
                out.add(("%sdeep_fwd<%s>" % (tag, "mid" if p["has_mid"] else "nomid"), dio))
            else:
                out.add(("%sdeep_inv<%s>" % (tag, ("mid%d%s" % (p["mid_inv"], ",compact" if p["compact"] else "")) if p["has_mid"] else "nomid"), dio))
            if p["flat"] and not (direction == "inv" and p["mid_inv"] == 2):
                out.add(("%sdeep_flat" % tag, dio))
    elif R["tail_l0"] >= 0:
        out.add(("tail", io))
    return {(f, direction, i) for f, i in out}


def seams(R):
    """(columns, rows) of the frame on which a job of any launched table begins -- strip seams, band seams with and without a link, the bands
    of the workgroup forms, the deep launch's deep / mid / flat split -- each with the sample before it; positions of deeper levels are
    scaled to the frame.  Keyed by tile origin: {(x0, y0): (cols, rows)} in the tile's own coordinates."""
    out = {}

    def add(x0, y0, l, col, row):
        cols, rows = out.setdefault((x0, y0), (set(), set()))
        if col > 0:
            cols.update(((col << l) - 1, col << l))
        if row > 0:
            rows.update(((row << l) - 1, row << l))

    for (l, cls), T in R["tabs"].items():
        if l >= R["nlaunch"]:
            continue
        for j in T.jobs + (T.pwg["jobs"] if T.pwg else []):
            x0, y0, _, _ = T.planes[j[0]]
            add(x0, y0, l, j[1], 2 * j[2])
    r8 = R["rgba8"]
    if r8:
        T = R["tabs"][(0, 1)]
        tables = [r8["pix_jobs"]]
        for k in ("fwd_wg", "inv_wg"):
            if r8[k]:
                tables.append(r8[k]["jobs"])
        if r8["fuse"]:
            tables += [r8["fuse"]["top"], r8["fuse"]["rest"]]
        if r8["mega"]:
            for d in ("fwd", "inv"):
                tables += [r8["mega"][d]["top"], [[j[0], 0, j[2], j[3], 0] for j in r8["mega"][d]["bands"]]]
        for tab in tables:
            for j in tab:
                x0, y0, _, _ = T.planes[j[0]]
                add(x0, y0, 0, j[1], 2 * j[2])
    for p in R["deep"]:
        for q in [p["T"], p["T1"], max(p["T1"] - 1, 0), min(p["T1"] + 1, p["T"])] + p["flat"]:
            add(p["x0"], p["y0"], R["deep_l0"], 0, 2 * q)
    return out


def seam_kinds(R):
    """how many band seams of the launched marching tables are linked through LDS and how many are not (every fourth band, and the bands too
    short to link)"""
    linked = unlinked = 0
    for (l, cls), T in R["tabs"].items():
        if l >= R["nlaunch"]:
            continue
        for j in T.jobs:
            if j[2] > 0:
                if j[4] & LINK_UP:
                    linked += 1
                else:
                    unlinked += 1
    return linked, unlinked


# ---- contents ---------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def impulse_points(W, H, tile, seam):
    """(y, x) in the frame: the corners of every tile, one sample in its last column and last row, one on every seam column and seam row"""
    pts = []
    for x0, y0, w, h in tiles_of(W, H, tile):
        cols, rows = seam.get((x0, y0), ((), ()))
        loc = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1), (h - 1, w // 2)]
        loc += [((7 * i + 3) % h, c) for i, c in enumerate(sorted(c for c in cols if c < w))]
        loc += [(r, (11 * i + 5) % w) for i, r in enumerate(sorted(r for r in rows if r < h))]
        pts += [(y0 + y, x0 + x) for y, x in loc]
    return list(dict.fromkeys(pts))


def int_frame(family, W, H, C, prec, seed=0, tile=(0, 0), seam=None):
    """an int32 frame [C, H, W] of unsigned `prec`-bit samples (`fullrange`: of any int32)"""
    rng = _rng(seed, W, H, C, prec, FRAME_FAMILIES.index(family))
    top, mid = (1 << prec) - 1, 1 << (prec - 1)
    yy, xx = np.mgrid[0:H, 0:W]
    if family == "noise":
        f = rng.integers(0, top + 1, size=(C, H, W))
    elif family == "fullrange":
        f = rng.integers(-2 ** 31, 2 ** 31, size=(C, H, W))
        lit = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31 + 1, 2 ** 30, -2 ** 30, -1, 0]
        f[C // 2].reshape(-1)[: min(W * H, 8)] = lit[: min(W * H, 8)]
    elif family == "const":
        f = np.stack([np.full((H, W), top if c % 2 == 0 else 0) for c in range(C)])
    elif family == "checker":
        f = np.stack([((xx + yy + c) & 1) * top for c in range(C)])
    elif family == "step":                      # a full-scale step on every seam column (component 0, 2, ...) / seam row (1, 2, ...) of every tile
        f = np.zeros((C, H, W), np.int64)
        for x0, y0, w, h in tiles_of(W, H, tile):
            cols, rows = (seam or {}).get((x0, y0), ((), ()))
            cs = sorted({c for c in cols if c < w and (c + 1) in cols} | {w // 2 - 1})
            rs = sorted({r for r in rows if r < h and (r + 1) in rows} | {h // 2 - 1})
            cx = np.zeros(w, np.int64)
            for c in cs:
                cx[c + 1:] ^= 1
            ry = np.zeros(h, np.int64)
            for r in rs:
                ry[r + 1:] ^= 1
            for c in range(C):
                v = np.zeros((h, w), np.int64)
                if c % 3 != 1:
                    v ^= cx[None, :]
                if c % 3 != 0:
                    v ^= ry[:, None]
                f[c, y0:y0 + h, x0:x0 + w] = v * top
    elif family == "impulse":                   # mid-grey (zero after the DC shift) with single full-scale samples
        f = np.full((C, H, W), mid, np.int64)
        for i, (y, x) in enumerate(impulse_points(W, H, tile, seam or {})):
            f[i % C, y, x] = top if i & 1 else 0
    else:
        raise ValueError(family)
    return np.asarray(f).astype(np.int64).astype(np.int32)


def step_edges(frame):
    """(columns, rows) c / r such that the frame changes between c and c + 1 / r and r + 1 somewhere"""
    f = np.asarray(frame, np.int64)
    return set(np.flatnonzero((f[:, :, 1:] != f[:, :, :-1]).any(axis=(0, 1)))), set(np.flatnonzero((f[:, 1:, :] != f[:, :-1, :]).any(axis=(0, 2))))


def coeff_plane(family, w, h, seed=0, cols=(), rows=()):
    """one tile-component's coefficients in the plane's Mallat layout (low halves first) that no forward transform produced; `impulse` puts a
    sample where a level-0 seam column / row lands in the low and in the high half"""
    rng = _rng(seed, w, h, 53, COEFF_FAMILIES.index(family))
    if family == "noise":
        f = rng.integers(-(1 << 12), 1 << 12, size=(h, w))
    elif family == "fullrange":
        f = rng.integers(-2 ** 31, 2 ** 31, size=(h, w))
        lit = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 30]
        f.reshape(-1)[: min(w * h, 6)] = lit[: min(w * h, 6)]
    elif family == "impulse":
        f = np.zeros((h, w), np.int64)
        hw, hh = (w + 1) // 2, (h + 1) // 2
        pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (hh - 1, hw - 1), (min(hh, h - 1), min(hw, w - 1))]
        for i, c in enumerate(sorted(c for c in cols if c < w)):
            y = (7 * i + 3) % h
            pts += [(y, c // 2), (y, min(hw + c // 2, w - 1))]
        for i, r in enumerate(sorted(r for r in rows if r < h)):
            x = (11 * i + 5) % w
            pts += [(r // 2, x), (min(hh + r // 2, h - 1), x)]
        for i, (y, x) in enumerate(dict.fromkeys(pts)):
            f[y, x] = (1 << 14) * (1 if i & 1 else -1)
    else:
        raise ValueError(family)
    return np.asarray(f).astype(np.int64).astype(np.int32)


def expect_forward(oracle, crop, prec, nres):
    """encoder.preprocess of one tile [C, h, w]"""
    C, h, w = crop.shape
    return np.stack(oracle.preprocess([np.ascontiguousarray(crop[c]) for c in range(C)], w, h, prec, True, nres))


def expect_inverse(oracle, coefs, prec, nres, is_signed=False):
    """the decode side of one tile [C, h, w]: tcd.ApplyInverseDWT per component, the inverse RCT on the first three, the DC shift (none for
    signed components, decoder.go:344-348)"""
    C, h, w = coefs.shape
    inv = [oracle.tcd_inverse_dwt(coefs[c], w, h, levels_of(nres), 1) for c in range(C)]
    return np.stack(oracle.postprocess(inv, prec, True, mct=C >= 3, is_signed=is_signed))


def out_of_range_rows(frame, prec):
    f = np.asarray(frame, np.int64)
    return ((f < 0) | (f > (1 << prec) - 1)).any(axis=(0, 2))


@functools.lru_cache(None)
def _pixelrange(w, h, C, prec, nres, seed):
    import oracle
    top = (1 << prec) - 1
    hh, hw = (h + 1) // 2, (w + 1) // 2
    for attempt in range(32):
        rng = _rng(seed, w, h, C, prec, nres, attempt, 555)
        base = rng.integers(top // 4, 3 * top // 4 + 1, size=(C, h, w)).astype(np.int32)
        co = expect_forward(oracle, base, prec, nres).astype(np.int64)
        amp = max(top // 64, 1)                     # every level-0 high-pass coefficient moves a little: not the transform of the base frame any more
        co[:, hh:, :] += rng.integers(-amp, amp + 1, size=(C, h - hh, w))
        co[:, :hh, hw:] += rng.integers(-amp, amp + 1, size=(C, hh, w - hw))
        nhp = h - hh                                # a high-pass row k of level 0 reaches the output rows 2k ... 2k + 2 and no other
        ks = sorted({(nhp // 3 + attempt) % nhp} | ({(2 * nhp // 3 + attempt) % nhp} if h >= 12 else set()))
        for k in ks:
            co[:, hh + k, :] += rng.choice([-1, 1], size=(C, w)) * rng.integers(2 * top, 6 * top, size=(C, w))
        co = co.astype(np.int32)
        bad = out_of_range_rows(expect_inverse(oracle, co, prec, nres), prec)
        if bad.sum() >= 2 and (~bad).sum() >= 2:
            co.setflags(write=False)
            return co
    raise AssertionError("no pixelrange set for %s" % ((w, h, C, prec, nres, seed),))


def pixelrange_set(w, h, C, prec, nres, seed=0):
    """coefficients [C, h, w] of one tile whose reconstruction leaves 0 ... 2^prec - 1 on two rows at least and stays inside it on two at least:
    the forward transform of an in-range frame, every level-0 high-pass coefficient moved a little, one or two high-pass rows moved by
    several times the range; the first of 32 seeded attempts on which the ORACLE's reconstruction has both kinds of row"""
    assert h >= PIXELRANGE_MIN_H
    return _pixelrange(w, h, C, prec, nres, seed)


def pack_pixels(fmt, frame, stride, pad_byte=0xA5):
    """a Go Pix buffer [H, stride] (image.Gray / Gray16 / RGBA / RGBA64 / NRGBA / NRGBA64: big-endian 16-bit samples) whose channels are the
    frame's components (a fourth, where the format has one and the frame does not, is opaque)"""
    Cf, H, W = frame.shape
    ch, bps = (1 if PIX_COMP[fmt] == 1 else 4), PIX_BPS[fmt]
    top = (1 << (8 * bps)) - 1
    px = np.full((H, W, ch), top, np.int64)
    px[..., : min(ch, Cf)] = np.asarray(frame, np.int64).transpose(1, 2, 0)[..., : min(ch, Cf)]
    px = np.clip(px, 0, top)
    if bps == 2:
        by = np.stack([px >> 8, px & 255], axis=-1).reshape(H, W * ch * 2)
    else:
        by = px.reshape(H, W * ch)
    out = np.full((H, stride), pad_byte, np.uint8)
    out[:, : by.shape[1]] = by.astype(np.uint8)
    return out


# ---- shapes, from the constants -----------------------------------------------------------------------------------------------------------
STRIP_BASES = (126, 128, 252, 256, 504, 512, 1008, 1016)    # 63 lanes of 2 / 4 / 8 columns, the first strips' widths, two strips of eight
STRIP_DELTAS = (-2, -1, 0, 1, 2, 4, 8)
WG_WIDTHS = (16, 24, 248, 504, 512)
WG_MULTI_WIDTHS = (520, 776, 1024, 1032)


def march_widths():
    ws = {b + d for b in STRIP_BASES for d in STRIP_DELTAS} | set(range(190, 197)) | set(range(380, 389)) | set(range(1, 10))
    return sorted(ws)


def march_heights():
    """1, 2, 3; one and two bands of band_prows and band_prows_pix pair-rows, one row less and more; the same around four bands (the workgroup
    seam without a link)"""
    d = defaults()
    hs = {1, 2, 3}
    for band in (d["band_prows"], d["band_prows_pix"]):
        hs |= {2 * band * k + e for k in (1, 2, 4) for e in (-1, 0, 1)}
    return sorted(hs)


@functools.lru_cache(None)
def march_shapes():
    """every width with a height, every height with three widths at least: planes of 1024 x 41 at the most"""
    ws, hs = march_widths(), march_heights()
    out = [(w, hs[(5 * i + 1) % len(hs)]) for i, w in enumerate(ws)]
    out += [(ws[(7 * i + 3 * k + 2) % len(ws)], h) for i, h in enumerate(hs) for k in range(3)]
    return tuple(dict.fromkeys(out))


def wg_heights(nr):
    halves = (nr - 1, nr, nr + 1, 2 * nr, 2 * nr + 1)
    return sorted({h for q in halves for h in (2 * q - 1, 2 * q) if h >= 2})


def fuse_heights(nr2):
    """levels 0 + 1 in one launch: bands of nr2 pair-rows of LEVEL 1 cover the top half; halfH1 = (halfH + 1) / 2 on, one below and one past
    the band, in both parities of the height"""
    halves1 = (nr2 - 1, nr2, nr2 + 1, 2 * nr2, 2 * nr2 + 1)
    return sorted({4 * q - 2 - e for q in halves1 for e in (0, 1)})


# ---- the case lists -------------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "group W H C tile prec nres env entry fmt pad")):
    """group: the test that runs it; env: the context's knobs; entry: frame / pixels / unit; fmt: the packed format of a pixels case; pad: bytes
    after every pixel row"""
    __slots__ = ()

    @property
    def id(self):
        knobs = "".join("-%s%d" % (k[4:].lower(), v) for k, v in self.env)
        f = "" if self.fmt is None else "-%s+%d" % (PIX_NAMES[self.fmt], self.pad)
        return "%s-%dx%dc%d-t%dx%d-p%d-r%d%s%s" % (self.group, self.W, self.H, self.C, self.tile[0], self.tile[1], self.prec, self.nres, f, knobs)

    @property
    def route(self):
        return route(self.W, self.H, self.C, self.tile, self.nres, self.env)

    @property
    def stride(self):
        if self.fmt is None:
            return 0
        return self.W * PIX_BYTES[self.fmt] + self.pad

    @property
    def out_stride(self):
        """of the image decoder.createImage makes of (components, precision)"""
        return self.W * (1 if self.C == 1 else 4) * (2 if self.prec > 8 else 1) + self.pad

    def forms(self, direction):
        if self.entry == "pixels":
            return forms(self.route, direction, "pixels", self.fmt, self.stride if direction == "fwd" else self.out_stride, self.prec)
        return forms(self.route, direction, self.entry)

    @property
    def pixelrange(self):
        return min(h for _, _, _, h in tiles_of(self.W, self.H, self.tile)) >= PIXELRANGE_MIN_H


def _env(**kw):
    return tuple(sorted(("J2K_" + k.upper(), int(v)) for k, v in kw.items()))


def _mk(group, W, H, C=1, tile=(0, 0), prec=8, nres=6, env=(), entry="frame", fmt=None, pad=0):
    return Case(group, W, H, C, tuple(tile), prec, nres, env, entry, fmt, pad)


@functools.lru_cache(None)
def marching_plane_cases():
    """one component, J2K_PLANE_WG=0, J2K_DEEP=0: dwt53_fwd_kernel / dwt53_inv_kernel<2 | 4 | 8, 1, vec | scalar> at every strip and band seam"""
    env = _env(plane_wg=0, deep=0)
    out = [_mk("march1", w, h, 1, (0, 0), PRECISIONS[i % 4], NRES[i % 6], env) for i, (w, h) in enumerate(march_shapes())]
    # tiled: a ragged last tile column and row; one whose ragged column of 6 drops the whole table to cpl 2 scalar; one whose column is 16 wide
    out += [_mk("march1", 520, 23, 1, (256, 10), 12, 3, env), _mk("march1", 518, 21, 1, (512, 0), 8, 2, env),
            _mk("march1", 528, 13, 1, (512, 6), 16, 4, env), _mk("march1", 1030, 9, 1, (1016, 0), 8, 0, env)]
    return tuple(out)


@functools.lru_cache(None)
def marching_rgb_cases():
    """three components (RCT + DC shift in the level-0 kernel), default options apart from J2K_DEEP=0: dwt53_*_kernel<cpl, 3, vec> for cpl 2 / 4
    / 8 and the scalar fallback; the deeper levels are single planes (workgroup form where admitted).  Four components: a single-plane table
    beside the triples'."""
    env = _env(deep=0)
    ws = sorted({b + d for b in (126, 128, 252, 256, 504, 512, 1008) for d in (-2, -1, 0, 1, 2, 4, 8)} | {1, 2, 3, 5, 8, 9, 190, 191, 192, 193, 196, 382, 383, 384, 385, 388})
    hs = march_heights()
    out = [_mk("march3", w, hs[(3 * i + 2) % len(hs)], 3, (0, 0), PRECISIONS[i % 4], NRES[(i + 2) % 6], env) for i, w in enumerate(ws)]
    out += [_mk("march3", ws[(11 * i + 4) % len(ws)], h, 3, (0, 0), PRECISIONS[(i + 1) % 4], NRES[i % 6], env) for i, h in enumerate(hs)]
    out += [_mk("march3", 512, 21, 4, (0, 0), 8, 3, env), _mk("march3", 253, 11, 4, (0, 0), 12, 2, env), _mk("march3", 130, 40, 4, (0, 0), 16, 4, env),
            _mk("march3", 386, 10, 4, (0, 0), 31, 0, env),
            _mk("march3", 520, 23, 3, (256, 10), 12, 3, env), _mk("march3", 518, 21, 3, (512, 0), 8, 2, env),
            _mk("march3", 528, 13, 3, (512, 6), 16, 4, env), _mk("march3", 1030, 9, 3, (1016, 0), 8, 0, env)]
    return tuple(dict.fromkeys(out))


@functools.lru_cache(None)
def plane_wg_cases():
    """J2K_PLANE_WG 4 and 8 (bands of 3 / 7 pair-rows): single planes of one strip and of several 512-column strips, RGB triples under
    J2K_PLANE_WG3=1, every level count; the 4096 pair-rows rule from both sides"""
    out = []
    for nw in (4, 8):
        env = _env(plane_wg=nw, deep=0)
        env3 = _env(plane_wg=nw, plane_wg3=1, deep=0)
        for i, h in enumerate(wg_heights(nw - 1)):
            out.append(_mk("pwg", WG_WIDTHS[i % 5], h, 1, (0, 0), PRECISIONS[i % 4], NRES[i % 6], env))
            out.append(_mk("pwg", WG_WIDTHS[(i + 2) % 5], h, 1, (0, 0), PRECISIONS[(i + 1) % 4], NRES[(i + 3) % 6], env))
            out.append(_mk("pwg", WG_MULTI_WIDTHS[i % 4], h, 1, (0, 0), PRECISIONS[(i + 2) % 4], NRES[(i + 1) % 6], env))
            out.append(_mk("pwg", (WG_WIDTHS + WG_MULTI_WIDTHS)[i % 9], h, 3, (0, 0), PRECISIONS[(i + 3) % 4], NRES[(i + 4) % 6], env3))
        out += [_mk("pwg", 528, 4 * nw - 3, 1, (512, 2 * nw), 12, 3, env), _mk("pwg", 1040, 2 * nw + 1, 3, (1024, 0), 8, 2, env3),
                _mk("pwg", 16, 8192, 1, (0, 0), 8, 3, env), _mk("pwg", 16, 8194, 1, (0, 0), 8, 3, env)]
    return tuple(out)


DEEP_VARIANTS = (dict(deep=0), dict(deep_mid=0, deep_mid_inv=0), dict(deep_mid=1, deep_mid_inv=0), dict(deep_mid=1, deep_mid_inv=1),
                 dict(deep_mid=1, deep_mid_inv=2))
# (W, H, C, tile): level 1 just misses and level 2 just fits the LDS rule (264, 260: no mid job / not a multiple of 4: the tail); level-l0 widths
# 256 / 252 / 128 / 8; T = 1, 2, 3, odd h1, halfH - T = 0, 1, 64 (65 needs h1 = 130: above the 256 rows the launch admits)
DEEP_TILES = ((264, 40, 3, (0, 0)), (260, 40, 3, (0, 0)), (512, 66, 1, (0, 0)), (512, 66, 3, (0, 0)), (504, 40, 1, (0, 0)), (256, 300, 1, (0, 0)),
              (528, 40, 3, (512, 0)), (512, 4, 3, (0, 0)), (512, 6, 1, (0, 0)), (512, 8, 3, (0, 0)), (512, 12, 3, (0, 0)), (512, 14, 1, (0, 0)),
              (512, 20, 3, (0, 0)), (512, 22, 1, (0, 0)), (512, 512, 1, (0, 0)), (264, 510, 3, (0, 0)), (512, 130, 3, (0, 0)), (1024, 37, 3, (512, 20)),
              (528, 36, 3, (512, 0)), (528, 24, 1, (512, 0)))       # a ragged column of 16: level-l0 width 8, odd h2 (mid job without the compact layout)
DEEP_NRES = (4, 6, 0, 5, 7, 3)      # 2 ... 5 levels inside the launch (l0 = 1); 3: two levels, neither a tail nor a deep launch


@functools.lru_cache(None)
def tail_deep_cases():
    """always J2K_DEEP_MIN_PLANES=1: the LDS tail (J2K_DEEP=0) and the deep launch with J2K_DEEP_MID 0 / 1 and J2K_DEEP_MID_INV 0 / 1 / 2"""
    out = []
    for v, var in enumerate(DEEP_VARIANTS):
        env = _env(deep_min_planes=1, **var)
        for i, (W, H, C, tile) in enumerate(DEEP_TILES):
            out.append(_mk("deep", W, H, C, tile, PRECISIONS[(i + v) % 4], DEEP_NRES[(i + v) % 6], env))
    return tuple(out)


RGBA8_KNOBS = ((), (("l0_wg", 0),), (("l0_wg", 4),), (("l0_wg_invw", 0),), (("l0_wg_invw", 8),), (("l0_wg_inv", 0),), (("l0_inv_wpe", 6),),
               (("l0_inv_wpe", 7),), (("l0_wg_invw", 8), ("l0_inv_wpe", 6)), (("l0_wg_invw", 8), ("l0_inv_wpe", 7)),
               (("l0_store", 0),), (("l0_store", 2),), (("l0_store", 4),), (("l0_fuse", 8),), (("l0_fuse", 10),), (("l0_fuse", 16),),
               (("l0_fuse", 8), ("l0_store", 0)), (("mega", 1), ("deep_min_planes", 1)), (("mega", 2), ("deep_min_planes", 1)))
# frames whose tiles are the workgroup widths 16 / 24 / 248 / 504 / 512: a table takes the RGBA8 forms only at eight columns per lane, so the
# narrow planes are ragged last tile columns
RGBA8_FRAMES = ((512, 0), (528, 512), (504, 0), (536, 512), (760, 512), (1008, 504))


@functools.lru_cache(None)
def rgba8_cases():
    """forward_rgba8 / inverse_rgba8 on packed RGBA8 pixels under every level-0 knob: heights around the bands of the forward form (l0_wg - 1
    pair-rows), of the inverse form, of the fused launch (l0_fuse - 3 pair-rows of level 1) and the merged launches' 15-row bands"""
    out = []
    for k, knobs in enumerate(RGBA8_KNOBS):
        o = dict(knobs)
        env = _env(**o)
        nrs = {(o.get("l0_wg", defaults()["l0_wg"]) or 1) - 1, (o.get("l0_wg_invw", defaults()["l0_wg_invw"]) or o.get("l0_wg", defaults()["l0_wg"]) or 1) - 1} - {0}
        hs = sorted({h for nr in (nrs or {3, 7}) for h in wg_heights(nr)})
        if not knobs:
            hs = sorted(set(wg_heights(3)) | set(wg_heights(7)) | {2, 3})
        if "l0_fuse" in o:
            hs = fuse_heights(o["l0_fuse"] - 3)
        if "mega" in o:
            hs = sorted(set(wg_heights(7)) | {3, 4, 61, 62, 63, 64, 91, 92, 122})     # split_row + 15 k on both sides
        for i, h in enumerate(hs):
            W, tw = RGBA8_FRAMES[(i + k) % 6]
            nres = (4, 6, 0, 5)[(i + k) % 4] if "mega" in o else (NRES[(i + k) % 6] if "l0_fuse" not in o else (2, 3, 4, 6, 0, 3)[(i + k) % 6])
            out.append(_mk("rgba8", W, h, 3, (tw, 0), 8, nres, env, "pixels", 2, (0, 16, 32)[(i + k) % 3]))
            if not knobs:
                W, tw = RGBA8_FRAMES[(i + 3) % 6]
                out.append(_mk("rgba8", W, h, 3, (tw, 0), 8, NRES[(i + 3) % 6], env, "pixels", 2, (16, 32, 0)[i % 3]))
    # rows that are not whole 16-byte lanes and a frame no table takes at eight columns per lane: staged through int32 planes
    out += [_mk("rgba8", 512, 14, 3, (0, 0), 8, 3, (), "pixels", 2, 4), _mk("rgba8", 200, 14, 3, (0, 0), 8, 3, (), "pixels", 2, 0),
            _mk("rgba8", 1024, 29, 3, (512, 15), 8, 4, (), "pixels", 2, 16)]
    return tuple(out)


PACKED_SHAPES = ((16, 0), (24, 0), (248, 0), (504, 0), (512, 0), (520, 0), (1024, 0), (528, 512), (776, 0))


@functools.lru_cache(None)
def packed_cases():
    """forward_pixels / inverse_pixels for the six formats through J2K_PIX_FUSE 0 / 1 / 2 at the shapes of the plane workgroup form (3 pair-rows
    at the default J2K_PLANE_WG=4): its SRC / DST 1 ... 4 instantiations; Gray16 and RGBA8 on the pixel-reading marching kernels"""
    out = []
    hs = wg_heights(defaults()["plane_wg"] - 1)
    for fmt in range(6):
        prec = 8 * PIX_BPS[fmt]
        for fuse in (0, 1, 2):
            env = _env(pix_fuse=fuse)
            n = 9 if fuse == 1 else 3
            for i in range(n):
                W, tw = PACKED_SHAPES[(i + fmt) % 9]
                pad = (-W * PIX_BYTES[fmt]) % 16 + (0, 16, 32)[(i + fmt) % 3]          # rows of whole 16-byte lanes: the kernels take the pixels themselves
                out.append(_mk("packed", W, hs[(3 * i + fmt + fuse) % len(hs)], PIX_COMP[fmt], (tw, 0), prec, NRES[(i + fmt) % 6], env, "pixels", fmt, pad))
    for i, (W, h) in enumerate(((512, 11), (504, 6), (1016, 31), (1024, 10))):           # Gray16 on dwt53_*_kernel<8, 1, true, PIX>
        out.append(_mk("packed", W, h, 1, (0, 0), 16, NRES[i % 6], _env(plane_wg=0), "pixels", 1, (0, 16)[i % 2]))
    for i, (W, h) in enumerate(((24, 13), (248, 14), (512, 15), (520, 12), (776, 27), (1024, 16))):    # Gray16 on the plane kernels at eight waves
        out.append(_mk("packed", W, h, 1, (0, 0), 16, NRES[(i + 1) % 6], _env(plane_wg=8), "pixels", 1, (0, 16, 32)[i % 3]))
    for i, (W, h) in enumerate(((512, 11), (504, 6), (528, 31), (1024, 10))):            # RGBA8 on dwt53_*_kernel<8, 3, true, PIX>
        out.append(_mk("packed", W, h, 3, (512, 0), 8, NRES[(i + 2) % 6], _env(l0_wg=0), "pixels", 2, (16, 0)[i % 2]))
    out += [_mk("packed", 100, 13, 4, (64, 0), 8, 3, (), "pixels", 4, 0), _mk("packed", 256, 12, 1, (0, 0), 8, 3, (), "pixels", 0, 8)]      # staged
    return tuple(out)


UNIT_WAVES = (0, 4, 8)
UNIT_LEVELS = (1, 3)


@functools.lru_cache(None)
def unit_shapes(nw):
    """the host unit calls run a cached one-component plan: under J2K_PLANE_WG=0 every marching shape, under 4 / 8 the shapes the form admits"""
    if nw == 0:
        return march_shapes()
    out = []
    for i, h in enumerate(wg_heights(nw - 1)):
        out += [(WG_WIDTHS[i % 5], h), (WG_WIDTHS[(i + 2) % 5], h), (WG_MULTI_WIDTHS[i % 4], h)]
    return tuple(out)


def unit_route(w, h, levels, nw):
    return route(w, h, 1, (0, 0), levels + 1, _env(plane_wg=nw))


def all_cases():
    return marching_plane_cases() + marching_rgb_cases() + plane_wg_cases() + tail_deep_cases() + rgba8_cases() + packed_cases()


def all_routes():
    """{route: [case ids]} over every case and both directions, the unit calls included"""
    out = collections.defaultdict(list)
    for c in all_cases():
        for d in ("fwd", "inv"):
            for r in c.forms(d):
                out[r].append(c.id)
    for nw in UNIT_WAVES:
        for w, h in unit_shapes(nw):
            for lv in UNIT_LEVELS:
                R = unit_route(w, h, lv, nw)
                for d in ("fwd", "inv"):
                    for r in forms(R, d, "unit"):
                        out[r].append("unit-wg%d-%dx%d-l%d" % (nw, w, h, lv))
    return dict(out)
