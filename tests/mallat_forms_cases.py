"""The cases of the specialised 5-3 forms a Mallat plan builds -- the packed-RGBA8 workgroup level 0 (dwt53_l0pix.inc) and single-component
planes in workgroup form at level 0 (dwt53_plane_wg.inc), the two that read / write packed pixels; the levels below keep the general Mallat
launches (the plane form below level 0 and the LDS tail were measured and did not pay: docs/KERNEL_NOTES.md) -- importable without a GPU: tests/test_mallat_forms_ref.py
checks on the CPU that every case has the level dimensions its comment claims, tests/test_gpu_mallat_forms.py runs them on the device.  The
expectation is tests/mallat_cases.py's; nothing here computes one.

FUSED is written down by hand from the contracts (pix_fusable in csrc/j2k_stages.cpp, the table contracts in csrc/j2k_planbuild.cpp), for a
pixel buffer whose base and stride are multiples of 16 bytes: does the level-0 launch read (forward) / write (inverse) the pixels itself?
A Mallat plan fuses where a prefix plan would AND that launch is a workgroup form."""
import lossless53_cases as ll
import mallat_cases as mc

# (W, H, components, precision, tile, resolutions)
CASES = (
    # RGBA8 workgroup level 0 (cpl = 8 needs a level-0 plane >= 384 wide).  halfH = 15: forward bands of 7 / 7 / 1 pair-rows, inverse of 3.
    # Below it 192 x 15 (odd height), 96 x 8, 48 x 4, 24 x 2: one general Mallat launch each.
    (384, 30, 3, 8, (0, 0), 6),
    # all 64 lanes live; odd H: the last pair-row has no odd row
    (512, 35, 3, 8, (0, 0), 4),
    # tile grid, edge tiles 16 wide and 12 high; level 1 has 8-wide planes beside a workgroup level 0
    (400, 44, 3, 8, (384, 32), 5),
    # edge tile 8 wide: no RGBA8 workgroup table, the pixels are staged
    (392, 20, 3, 8, (384, 0), 3),
    # Gray16, three strips (512, 512, 16): the multi-strip plane kernel
    (1040, 10, 1, 16, (0, 0), 3),
    # Gray8, partly idle wave; odd height, 32 x 11 below
    (64, 21, 1, 8, (0, 0), 4),
    # RGBA64 through the plane kernel, NC = 3
    (64, 20, 3, 16, (0, 0), 3),
    # NRGBA: RGBA8 triple kernel plus the alpha plane's read-modify-write store (DST 3)
    (384, 12, 4, 8, (0, 0), 3),
    # NRGBA64
    (64, 12, 4, 16, (0, 0), 3),
    # no pixel format: planar int32 in and out, general launches throughout (the triple's plane table serves pixel sources only)
    (384, 16, 3, 12, (0, 0), 4),
)

# case -> (forward, inverse), None: the case has no pixel format
#  1 - 3   every level-0 plane is 16 ... 512 wide, a multiple of 8, two rows at least: both RGBA8 workgroup tables exist (8 / 4 waves, the defaults)
#  4       the 8-wide edge tile fails `w >= 16`: no table; a prefix plan would fuse through the general kernel, a Mallat plan has none for pixels
#  5, 6    one component: the plane-workgroup table of level 0 (w % 8 == 0, w >= 16, h >= 2, W % 8 == 0; Gray8 needs plane_wg = 4, the default)
#  7       the triple's plane table (kept for pixel sources), four waves
#  8, 9    the triple as in 1 / 7, the alpha plane through the single-plane table: one single plane beside the triple, so the inverse's
#          read-modify-write of its channel is safe
FUSED = ((1, 1), (1, 1), (1, 1), (0, 0), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), None)

# Case 1, j2k_ctx_profile_enable(2): dispatches per tag (0 forward level 0, 1 forward deeper levels, 2 inverse level 0, 3 inverse deeper levels) of
# one forward_pixels and one inverse_pixels.  Level 0 is the RGBA8 workgroup launch (with the options off: the general one); below it one
# general launch per level, the three planes of a level together.
DISPATCHES_CASE1 = {0: 1, 1: 4, 2: 1, 3: 4}


def case_id(c):
    return mc.case_id(c)


def pix_format(case):
    return mc.PIX_FORMAT.get((case[2], case[3]))


def bpp(case):
    return (1 if case[2] == 1 else 4) * (2 if case[3] > 8 else 1)


def level_dims(case):
    """per tile (x0, y0, w, h): [(w_0, h_0), ..., (w_L, h_L)]"""
    W, H, _, _, tile, nres = case
    return {(x0, y0, w, h): mc.dims(w, h, mc.levels_of(nres)) for x0, y0, w, h in ll.tiles_of(W, H, tile)}


def wg_contract(w, h):
    """the geometry contract of the plane-workgroup kernels; the RGBA8 ones add w <= 512"""
    return w >= 16 and w % 8 == 0 and h >= 2


def seam_map(case):
    """mallat_cases.seam_map plus the band rows of the workgroup forms (bands of waves - 1 pair-rows: RGBA8 forward, RGBA8 inverse, planes)
    and column 512, where a plane's second strip begins"""
    W, H, _, _, tile, nres = case
    d = ll.defaults()
    out = {}
    for key, (cols, rows) in mc.seam_map(W, H, tile, nres).items():
        w, h = next((w, h) for x0, y0, w, h in ll.tiles_of(W, H, tile) if (x0, y0) == key)
        rows = set(rows)
        for waves in (d["l0_wg"], d["l0_wg_invw"], d["plane_wg"]):
            rows |= {r + e for r in range(2 * (waves - 1), h, 2 * (waves - 1)) for e in (-1, 0)}
        cols = set(cols) | {c for c in (511, 512) if c < w}
        out[key] = (tuple(sorted(cols)), tuple(sorted(rows)))
    return out


def frame(case, family, seed=0):
    W, H, Cn, prec, tile, _ = case
    return ll.int_frame(family, W, H, Cn, prec, seed, tile, seam_map(case))
