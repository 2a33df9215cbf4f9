// plan_tables.cpp -- a frame geometry compiled into job tables (plan_tables.h): which workgroup touches which rows of which plane, for every
// kernel form.  Plain integer code, no HIP: build_plan (j2k_planbuild.cpp) uploads what this makes.
#include "plan_tables.h"

#include <algorithm>
#include <map>
#include <tuple>

namespace j2k {

bool PlanSpec::operator==(const PlanSpec &o) const {
    return W == o.W && H == o.H && C == o.C && tile_w == o.tile_w && tile_h == o.tile_h && levels == o.levels &&
           frame_h == o.frame_h && wavelet == o.wavelet && precision == o.precision && dc_shift == o.dc_shift && dc_shift_inv == o.dc_shift_inv && mct == o.mct && quant == o.quant && quality == o.quality &&
           num_res_jobs == o.num_res_jobs && cb_w == o.cb_w && cb_h == o.cb_h && coder == o.coder &&
           tile_first == o.tile_first && tile_count == o.tile_count && frame_is_f64 == o.frame_is_f64 && closed_loop == o.closed_loop && mallat == o.mallat;
}

}  // namespace j2k

using namespace j2k;

extern "C" size_t j2k_block_bound(int coder, int w, int h) {
    size_t n = (size_t)std::max(w, 0) * (size_t)std::max(h, 0);
    if (coder == J2K_CODER_HT) {               // ht.go:969-996: MagSgn + MEL + VLC buffers + SCUP
        size_t maxSize = std::max<size_t>(n * 2, 64);
        return maxSize / 2 + maxSize / 4 + maxSize / 2 + 2;
    }
    // t1_fast5.go:47-56: mqBuf has width*height*2 + 1024 bytes but never fewer than 16384 (a fresh T1; a pooled one may have
    // more left over from a larger block, which is history, not geometry).  A block that needs more than this is an index
    // panic in the reference; one that fits must be coded: the 16384 floor matters for deep 64x64 blocks (16-bit noise
    // after five lifting levels is ~9.3 KB against 2wh + 1024 = 9216; found by tools/fuzz_gpu.py).
    return std::max<size_t>(n * 2 + 1024, 16384);
}

namespace {

typedef std::vector<DwtJob> Jobs;
const DwtJob PAD_JOB = {-1, 0, 0, 0};

inline int64_t align4(int64_t v) { return (v + 3) & ~int64_t(3); }
inline int half(int v) { return (v + 1) / 2; }

// ------------------------------------------------------------------------------
// shared helpers: level dimensions, bands, the workgroup forms' geometry contract, XCD orders
// ------------------------------------------------------------------------------
struct Dim { int w, h; };
Dim level_dim(int w, int h, int l) {      // a w x h tile-component at the input of level l
    for (int i = 0; i < l; i++) { w = half(w); h = half(h); }
    return Dim{w, h};
}
// the first level 1 ... max_l0 whose input fits the LDS buffers in every group, or -1
int first_lds_level(const std::vector<Group> &groups, int max_l0) {
    for (int l0 = 1; l0 <= max_l0; l0++) {
        bool fits = true;
        for (const Group &g : groups) {
            const Dim d = level_dim(g.w, g.h, l0);
            if (d.w > 128 || (int64_t)d.w * d.h > 16384) fits = false;
        }
        if (fits) return l0;
    }
    return -1;
}

// bands of nr pair-rows of one plane over the pair-rows [from, to), ncol entries each (col0, col0 + 1, ...); returns the first pair-row not covered
int add_bands(Jobs &jobs, int plane, int from, int to, int nr, int col0 = 0, int ncol = 1) {
    int pr = from;
    for (; pr < to; pr += nr)
        for (int k = 0; k < ncol; k++) jobs.push_back(DwtJob{plane, col0 + k, pr, nr});
    return pr;
}

// the geometry contract of the workgroup forms: whole 16-byte lanes, at least two rows, and (unless the form cuts 512-column strips) one strip
bool wg_geometry(int w, int h, bool strips = false) { return !(w < 16 || (!strips && w > 512) || (w % 8) || h < 2); }
// 16-byte vector accesses at every offset of a plane
bool offsets_aligned(const DwtPlane &D) {
    for (int k = 0; k < 3; k++)
        if ((D.src_off[k] % 4) || (D.out_off[k] % 4) || (D.nxt_off[k] % 4)) return false;
    return true;
}

// XCD-aware orders for per-workgroup job tables: workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one), in table order.  Speed only.
// One contiguous chunk of the table per XCD: workgroup b takes job (b % 8) * chunk + b / 8: vertically adjacent bands -- which share three
// halo rows -- run on one XCD at about the same time and the re-read is an L2 hit.
void xcd_chunked(Jobs &v) {
    const size_t chunk = (v.size() + 7) / 8;
    Jobs perm(chunk * 8, PAD_JOB);
    for (size_t b = 0; b < perm.size(); b++) {
        const size_t j = (b % 8) * chunk + b / 8;
        if (j < v.size()) perm[b] = v[j];
    }
    v.swap(perm);
}
// Each XCD gets a contiguous chunk of the FULL bands (neighbouring bands share halo rows: L2 hits) followed by a chunk of the SHORT ones (the last
// band of a plane, fewer live waves: those whose nr pair-rows reach past the plane's, heights ph): a frame whose full bands fill the device a whole
// number of times then ends with the short workgroups instead of one more round of full ones (4K, 512-tiles, 5-row bands: 2040 full + 40 short
// workgroups on 512 slots).
void xcd_dealt(Jobs &wj, int nr, const std::vector<int> &ph) {
    Jobs full, shrt;
    for (const DwtJob &j : wj) (j.prow0 + nr > half(ph[j.plane]) ? shrt : full).push_back(j);
    std::vector<Jobs> per(8);
    for (Jobs *v : {&full, &shrt}) {
        const size_t chunk = (v->size() + 7) / 8;
        for (size_t i = 0; i < v->size(); i++) per[i / std::max<size_t>(chunk, 1)].push_back((*v)[i]);
    }
    size_t m = 0;
    for (auto &v : per) m = std::max(m, v.size());
    Jobs perm(m * 8, PAD_JOB);
    for (int x = 0; x < 8; x++)
        for (size_t i = 0; i < per[x].size(); i++) perm[i * 8 + x] = per[x][i];
    wj.swap(perm);
}
// In small groups: G consecutive bands (which share halo rows) go to ONE XCD, one after the other, and the eight XCDs work on eight
// neighbouring groups at a time -- the halo re-reads still hit that XCD's L2 (G - 1 of G boundaries) while the device as a whole sweeps
// memory in order, as the plain job order does (tools/probe/l0_inv_probe.hip: 5.7 TB/s in plain order, 5.4-5.5 in any order that gives
// every XCD a region of its own).  Table position p runs on XCD p % 8.
void xcd_grouped(Jobs &wj, size_t G) {
    const size_t ng = (wj.size() + G - 1) / G, rows = (ng + 7) / 8 * G;
    Jobs perm(rows * 8, PAD_JOB);
    for (size_t g = 0; g < ng; g++)
        for (size_t j = 0; j < G && g * G + j < wj.size(); j++) perm[((g / 8) * G + j) * 8 + g % 8] = wj[g * G + j];
    wj.swap(perm);
}
// The general kernels' tables (option xcd_map; four wavefront jobs per workgroup): the wavefronts of one plane -- whose bands share halo
// rows -- are placed in workgroups = x (mod 8): the halo re-reads then hit that XCD's L2 instead of going back to HBM.
void xcd_by_plane(Jobs &jobs) {
    std::vector<Jobs> per(8);
    for (const DwtJob &j : jobs) per[j.plane % 8].push_back(j);
    size_t m = 0;
    for (auto &v : per) m = std::max(m, v.size());
    m = (m + 3) & ~size_t(3);
    Jobs perm(m * 8, PAD_JOB);
    for (int x = 0; x < 8; x++)
        for (size_t i = 0; i < per[x].size(); i++) perm[((i / 4) * 8 + x) * 4 + (i % 4)] = per[x][i];
    jobs.swap(perm);
}

// ------------------------------------------------------------------------------
// tile-components, coefficient + scratch offsets
// ------------------------------------------------------------------------------
void tile_components(const PlanSpec &S, PlanTables &T) {
    // a batch (j2k_params.frame_rows): S.H / fh frames stacked vertically, the tile grid starts again at every frame
    const int fh = S.frame_h > 0 ? S.frame_h : S.H;
    const int tw = S.tile_w > 0 ? S.tile_w : S.W, th = S.tile_h > 0 ? S.tile_h : fh;
    const int tiles_y_frame = (fh + th - 1) / th;
    T.tiles_x = (S.W + tw - 1) / tw;
    T.tiles_y = tiles_y_frame * (S.H / fh);
    const int ntiles_all = T.tiles_x * T.tiles_y;
    T.tile_first = std::min(std::max(S.tile_first, 0), ntiles_all);
    T.tile_count = S.tile_count > 0 ? std::min(S.tile_count, ntiles_all - T.tile_first) : ntiles_all - T.tile_first;
    const bool triple = S.mct && S.C >= 3;
    int64_t coef = 0, sa = 0, sb = 0;
    for (int tl = 0; tl < T.tile_count; tl++) {
        const int t = T.tile_first + tl;
        const int tx = t % T.tiles_x, ty = t / T.tiles_x;
        const int x0 = tx * tw, y0 = (ty / tiles_y_frame) * fh + (ty % tiles_y_frame) * th;
        const int w = std::min(tw, S.W - x0), h = std::min(th, fh - (ty % tiles_y_frame) * th);
        const Dim d1 = level_dim(w, h, 1), d2 = level_dim(w, h, 2);
        int c = 0;
        while (c < S.C) {
            Group g{};
            g.tile = tl; g.comp0 = c; g.nc = (triple && c == 0) ? 3 : 1;
            g.x0 = x0; g.y0 = y0; g.w = w; g.h = h;
            for (int k = 0; k < g.nc; k++) {
                g.coef_off[k] = coef; coef += align4((int64_t)w * h);
                g.scrA_off[k] = sa; sa += align4((int64_t)d1.w * d1.h);
                g.scrB_off[k] = sb; sb += align4((int64_t)d2.w * d2.h);
                const int64_t d[7] = {t, c + k, x0, y0, w, h, g.coef_off[k]};
                T.plane_desc.insert(T.plane_desc.end(), d, d + 7);
            }
            T.groups.push_back(g);
            c += g.nc;
        }
    }
    T.coeff_elems = coef; T.scrA_elems = sa; T.scrB_elems = sb;
}

// ------------------------------------------------------------------------------
// fused LDS tail for the small levels (5-3 only)
// ------------------------------------------------------------------------------
void lds_tail(const PlanSpec &S, PlanTables &T) {
    const int L = S.levels, l0 = first_lds_level(T.groups, L - 2);
    if (l0 < 0) return;
    T.tail_l0 = l0;
    for (const Group &g : T.groups) {
        const Dim d = level_dim(g.w, g.h, l0), d1 = level_dim(d.w, d.h, 1), d2 = level_dim(d.w, d.h, 2);
        T.tail_lds_fwd = std::max(T.tail_lds_fwd, (size_t)(((d.w * d.h + 3) & ~3) + d1.w * d1.h + 8) * 4);
        T.tail_lds_inv = std::max(T.tail_lds_inv, (size_t)(((d1.w * d1.h + 3) & ~3) + d2.w * d2.h + 8) * 4);
        for (int k = 0; k < g.nc; k++) {
            TailPlane P{};
            P.scr_off = ((l0 & 1) ? g.scrA_off : g.scrB_off)[k];   // where level l0's input prefix lives
            P.coef_off = g.coef_off[k];
            P.w = d.w; P.h = d.h; P.nlev = L - l0;
            T.tail.push_back(P);
        }
    }
    T.ntail = (int)T.tail.size();
}

// ------------------------------------------------------------------------------
// every level below level 0 in one launch per direction (dwt53_deep.inc)
// ------------------------------------------------------------------------------
// the deep / mid jobs and the flat ones of both directions, before they become the launch's table (the merged launches put level-0 bands between them)
struct DeepRoles { Jobs deep[2], flat[2]; size_t lds_fwd = 0, lds_inv = 0; };

// One plane's share: the LDS both launches need for a w x h plane of level l0, and its jobs.  The forward and the inverse launch: the deep and
// mid jobs own different level-l0 rows.  false: the plane breaks the launch's contract.
bool deep_plane(const PlanOptions &o, int nlev, int w, int h, int pi, int ncopies, DeepRoles &R) {
    if (w < 8 || w > 256 || (w % 4) || h < 2 || h > 256) return false;
    const int w1 = w / 2, h1 = half(h), w2 = half(w1), h2 = half(h1);
    if (w1 > 128 || (int64_t)w1 * h1 > 16384) return false;
    const int halfH = h1, Tp = half(halfH), T1 = half(Tp);   // pair-rows of level l0; of level l0+1; those feeding level l0+2
    // the top half split once more (dwt53_deep.inc): level l0+1 must take the pair-column LDS routines, whole 16-byte runs
    const bool has_mid = o.deep_mid && Tp >= 2 && (w % 8) == 0 && (w1 & 1) == 0 && (64 % (w1 / 2)) == 0 && h1 >= 2;
    const size_t a_ints = has_mid ? (size_t)(2 * T1 + 2) * w1 : (size_t)w1 * h1;
    const size_t n1a = (a_ints + 3) & ~size_t(3), n2a = (size_t)((w2 * h2 + 3) & ~3), nc = (size_t)((w1 * h1 + 3) & ~3), slots = 16 * 64 * 4;   // (ints)
    R.lds_fwd = std::max(R.lds_fwd, (std::max(2 * slots, n2a) + n1a + 8) * 4);          // forward: slotE, slotD (later bufB) | bufA
    const size_t n1i = (has_mid && o.deep_mid_inv) ? n1a : nc;                          // (the inverse takes the split only on request)
    // inverse, deep + mid + flat (J2K_DEEP_MID_INV=1, the default since round 4): the staged coefficients as compact runs in the
    // places that are free when they are needed (dwt53_deep_inv_body, DEEP_COMPACT) -- bufA | X = bufB + the low-pass rows beyond
    // |X_{l0+2}| (mid: its low-pass rows) | RB = the high-pass rows: 69 KB for a 256 x 256 plane instead of 113, two workgroups per CU
    const size_t nn1 = (nlev > 2) ? (size_t)w2 * h2 : 0;
    const bool compact = has_mid && o.deep_mid_inv == 1 && (w1 % 4) == 0 && (nn1 % 4) == 0;
    if (compact) {
        const size_t lowtail = (size_t)std::max<int64_t>((int64_t)std::min(T1 + 2, Tp) * w1 - (int64_t)nn1, 0), lowmid = (size_t)(Tp - T1) * w1;
        const size_t xsize = (std::max(std::max(n2a + lowtail, lowmid), slots) + 3) & ~size_t(3);
        const size_t rb = (size_t)std::max(std::min(Tp + T1 + 2, h1) - Tp, h1 - (Tp + T1 - 1)) * w1;
        R.lds_inv = std::max(R.lds_inv, (n1a + xsize + rb + 8) * 4);
    } else
        R.lds_inv = std::max(R.lds_inv, (n1i + n2a + std::max(nc, slots) + 8) * 4);     // inverse: bufA | bufB | bufC (= slotE later)
    const int flag = has_mid ? 0x10000 : 0;
    const int cflag = compact ? 0x20000 : 0;
    // The inverse launch cannot share a CU between two workgroups (113 KB of LDS, 95 registers), so a third job per
    // plane waits for a CU and the split gains nothing there (J2K_DEEP_MID_INV: 0 = deep + flat, 16.2 us on a C2 frame;
    // 1 = deep + mid + flat, 16.5; 2 = deep + mid, each rebuilding half of the bottom rows first, 18.2).  The forward
    // launch fits two per CU (65 KB, 64 registers): 16.3 -> 13.8 us.
    const int mid_inv = has_mid ? o.deep_mid_inv : 0;
    for (int k = 0; k < ncopies; k++, pi++) {
        if (has_mid) {
            R.deep[0].push_back(DwtJob{pi, 1, 0, std::min(T1 + 1, Tp) | flag});
            R.deep[0].push_back(DwtJob{pi, 3, T1 - 1, (Tp - (T1 - 1)) | flag});
        } else R.deep[0].push_back(DwtJob{pi, 1, 0, Tp});
        if (mid_inv == 2) {
            const int nf = halfH - Tp, fa = half(nf);
            R.deep[1].push_back(DwtJob{pi, 1 | fa << 8, 0, T1 | flag});
            R.deep[1].push_back(DwtJob{pi, 3 | (nf - fa) << 8 | fa << 16, T1, (Tp - T1) | flag});
        } else if (mid_inv == 1) {
            R.deep[1].push_back(DwtJob{pi, 1, 0, T1 | flag | cflag});
            R.deep[1].push_back(DwtJob{pi, 3, T1, (Tp - T1) | flag | cflag});
        } else R.deep[1].push_back(DwtJob{pi, 1, 0, Tp});
        for (int q = Tp; q < halfH; q += 64) {
            R.flat[0].push_back(DwtJob{pi, 0, q, std::min(64, halfH - q)});
            if (mid_inv != 2) R.flat[1].push_back(DwtJob{pi, 0, q, std::min(64, halfH - q)});
        }
    }
    return true;
}

// levels deep_l0 .. L-1, deep_l0 = the level above the first one that fits LDS (lds_l0): it streams from memory in the same workgroups
void deep_launch(const PlanOptions &o, const PlanSpec &S, int lds_l0, PlanTables &T, DeepRoles &R) {
    const int L = S.levels, l0 = lds_l0 - 1;
    bool ok = true;
    std::vector<TailPlane> tp;
    for (const Group &g : T.groups) {
        const Dim d = level_dim(g.w, g.h, l0);
        if (!deep_plane(o, L - l0, d.w, d.h, (int)tp.size(), g.nc, R)) { ok = false; break; }
        for (int k = 0; k < g.nc; k++) {
            const int64_t so = ((l0 & 1) ? g.scrA_off : g.scrB_off)[k];
            if ((so % 4) || (g.coef_off[k] % 4)) ok = false;
            TailPlane P{};
            P.scr_off = so; P.coef_off = g.coef_off[k];
            P.w = d.w; P.h = d.h; P.nlev = L - l0;
            tp.push_back(P);
        }
    }
    // One deep chain per plane: with a handful of planes (C5: one 2048 x 2048 plane per frame) the per-level launches, which
    // spread every level over the whole device, are at least as fast (C5 at eight frames in flight: 76 Gpixel/s with the chain, 72-80 without)
    if (ok && (int)tp.size() < o.deep_min_planes) ok = false;
    if (!ok || tp.empty()) { R = DeepRoles(); return; }
    // deep jobs first (the longest chains), mid jobs behind them, then the flat ones
    auto order = [](Jobs d, const Jobs &f) {
        std::stable_sort(d.begin(), d.end(), [](const DwtJob &a, const DwtJob &b) { return (a.col0 & 0xff) < (b.col0 & 0xff); });
        d.insert(d.end(), f.begin(), f.end());
        return d;
    };
    T.deep_jobs = order(R.deep[0], R.flat[0]); T.deep_jobs_inv = order(R.deep[1], R.flat[1]);
    T.deep_planes.swap(tp);
    T.deep_l0 = l0; T.ndeep_jobs = (int)T.deep_jobs.size(); T.ndeep_jobs_inv = (int)T.deep_jobs_inv.size(); T.deep_lds = R.lds_inv; T.deep_lds_fwd = R.lds_fwd;
}

// ------------------------------------------------------------------------------
// one level of one class of groups: its planes and the kernel instantiation its tables are cut for
// ------------------------------------------------------------------------------
inline int pick_cpl(int maxw) { return maxw >= 384 ? 8 : (maxw >= 192 ? 4 : 2); }

// the frame a level reads (forward) / writes (inverse): W x H, tile (x0, y0) at (x0 >> shift, y0 >> shift) -- the plan's own frame, or the reduced one
struct FrameDst { int W, H, shift; };
struct Level {
    int dir = 0, l = 0, cls = 0;
    std::vector<DwtPlane> planes;
    std::vector<int> pw, ph, pnc;       // per plane: dims at this level, components in the plane (3 = a triple)
    int maxw = 0;
    bool vec_ok = true;                 // what the planes' own geometry leaves of it
    int cpl = 2, halo = 1;              // (level_rule)
};

// The planes of level l of every group of class cls (-1: both, in group order).  `final`: the level reads / writes frame F and takes MCT triples
// as one plane (level 0; the last launch of a reduced decode); else its input / output is a scratch prefix and every component a plane.
Level level_planes(const PlanSpec &S, const std::vector<Group> &groups, int dir, int l, int cls, bool final, const FrameDst &F, bool vec_ok) {
    Level Lv;
    Lv.dir = dir; Lv.l = l; Lv.cls = cls; Lv.vec_ok = vec_ok;
    const bool mal = S.mallat;
    for (const Group &g : groups) {
        const bool as_triple = (g.nc == 3 && final);
        if (cls >= 0 && (cls == 1) != as_triple) continue;
        const Dim d = level_dim(g.w, g.h, l), dn = level_dim(d.w, d.h, 1);
        const int nplanes_here = as_triple ? 1 : g.nc;
        if (mal && (g.w % 4)) Lv.vec_ok = false;      // rows of the coefficient plane are 16-byte aligned only then
        for (int k0 = 0; k0 < nplanes_here; k0++) {
            DwtPlane D{};
            const int kn = as_triple ? 3 : 1;
            for (int k = 0; k < kn; k++) {
                const int kk = as_triple ? k : k0;
                const int64_t frame_off = (int64_t)(g.comp0 + kk) * F.H * F.W + (int64_t)(g.y0 >> F.shift) * F.W + (g.x0 >> F.shift);
                const int64_t *scr_in = (l & 1) ? g.scrA_off : g.scrB_off;    // where level l's input prefix lives
                const int64_t *scr_out = (l & 1) ? g.scrB_off : g.scrA_off;   // where level l's output prefix goes
                if (dir == 0) {  // forward
                    D.src_off[k] = final ? frame_off : scr_in[kk];
                    D.out_off[k] = g.coef_off[kk];
                    D.nxt_off[k] = scr_out[kk];
                } else {         // inverse: X_l lives where the forward input of level l lived
                    D.src_off[k] = g.coef_off[kk];
                    D.nxt_off[k] = scr_out[kk];               // X_{l+1}
                    D.out_off[k] = final ? frame_off : scr_in[kk];
                }
            }
            D.src_stride = (dir == 0 && final) ? F.W : d.w;
            D.out_stride = F.W;
            D.w = d.w; D.h = d.h;
            D.n_next = (l == S.levels - 1) ? 0 : dn.w * dn.h;
            D.coef_stride = mal ? g.w : 0;
            Lv.planes.push_back(D);
            Lv.pw.push_back(d.w); Lv.ph.push_back(d.h); Lv.pnc.push_back(kn);
            Lv.maxw = std::max(Lv.maxw, d.w);
        }
    }
    return Lv;
}

// Which instantiation of the general kernels a level table is cut for: columns per lane, vector accesses or not, halo lanes per side.  One
// rule for the plan's level tables and for the final launch of a reduced decode: the job table and the launch must agree on it.
//   frame_stride > 0: the level reads / writes a frame with this row stride (level 0; the final launch of a reduced decode)
//   cpl0: the J2K_CPL0 tuning knob (5-3 level 0), 0 = none;  Lv.vec_ok: what the caller has ruled out already
void level_rule(const PlanSpec &S, Level &Lv, int frame_stride, int cpl0, LevelInfo &T) {
    int cpl = pick_cpl(Lv.maxw);
    bool vec_ok = Lv.vec_ok;
    if (cpl0 > 0 && S.wavelet == W53) cpl = cpl0;
    if (S.wavelet == W97) cpl = (Lv.cls == 1) ? 2 : (Lv.maxw >= 192 ? 4 : 2);   // f64: 2 or 4 columns per lane
    for (size_t i = 0; i < Lv.planes.size() && vec_ok; i++) {
        const DwtPlane &D = Lv.planes[i];
        if (D.w % cpl) vec_ok = false;
        if (frame_stride > 0 && (frame_stride % cpl)) vec_ok = false;
        if (!offsets_aligned(D)) vec_ok = false;
    }
    if (S.wavelet == W97) vec_ok = false;        // the 9-7 kernels use scalar accesses
    else if (!vec_ok) cpl = 2;
    Lv.cpl = cpl; Lv.vec_ok = vec_ok;
    Lv.halo = (S.wavelet == W97 && cpl < 4) ? 2 : 1;      // lanes per side that only feed their neighbours (1 for 5-3; 9-7: 1 if a lane holds >= 2 pairs, else 2)
    T.cpl = cpl; T.vec = vec_ok ? 1 : 0;
}

// ------------------------------------------------------------------------------
// the general level tables: one wavefront per (64-lane column strip, band of pair-rows)
// ------------------------------------------------------------------------------
Jobs general_jobs(const Level &Lv, int band) {
    Jobs jobs;
    for (size_t i = 0; i < Lv.planes.size(); i++) {
        const int w = Lv.pw[i], cpl = Lv.cpl;
        for (int col0 = 0;;) {
            const int c_base = col0 - (col0 ? Lv.halo * cpl : 0);
            add_bands(jobs, (int)i, 0, std::max(half(Lv.ph[i]), 1), band, col0);
            if (c_base + 64 * cpl >= w) break;
            col0 = c_base + (64 - Lv.halo) * cpl;
        }
    }
    return jobs;
}
// link vertically adjacent bands that share a workgroup (4 consecutive jobs): see dwt53_fwd_kernel
void link_bands(const Level &Lv, Jobs &jobs) {
    for (size_t i = 1; i < jobs.size(); i++) {
        if (i % 4 == 0) continue;
        DwtJob &a = jobs[i - 1], &b = jobs[i];
        if (a.plane < 0 || a.plane != b.plane || a.col0 != b.col0) continue;
        const int w = Lv.pw[a.plane], h = Lv.ph[a.plane], halfH = half(h);
        if (w < 2 || h < 2) continue;
        const int an = a.nprow & 0xffff, bn = b.nprow & 0xffff;
        if (a.prow0 + an != b.prow0) continue;
        if (std::min(an, halfH - a.prow0) < 2 || std::min(bn, halfH - b.prow0) < 2) continue;
        if (2 * b.prow0 + 1 >= h) continue;      // the band below must own a real odd row
        a.nprow |= J2K_LINK_DOWN;
        b.nprow |= J2K_LINK_UP;
    }
}
// ... in the plan's order: XCD-aware on request, linked where the 5-3 kernels link
Jobs level_jobs(const PlanOptions &o, const PlanSpec &S, const Level &Lv, int band) {
    Jobs jobs = general_jobs(Lv, band);
    if (o.xcd_map && jobs.size() >= 64) xcd_by_plane(jobs);
    if (S.wavelet == W53 && (Lv.dir == 0 ? o.fwd_link : o.inv_link)) link_bands(Lv, jobs);
    return jobs;
}
int general_band(const PlanOptions &o, const PlanSpec &S, int dir) {
    const int band53 = (dir == 1 && o.band_prows_inv > 0) ? o.band_prows_inv : o.band_prows;
    return (S.wavelet == W97) ? o.band_prows_97 : band53;
}

// ------------------------------------------------------------------------------
// single-component planes in workgroup form: 5-3 (dwt53_plane_wg.inc) and 9-7
// ------------------------------------------------------------------------------
// 5-3, both directions: whole 16-byte lanes, at least two rows
// (a Mallat plan: level 0 only, where the form reads / writes the packed pixels.  vec_ok holds the rule that every tile-component
//  of the table is a multiple of 4 wide, so the rows of its coefficient plane are 16-byte aligned; w % 8 == 0 makes the
//  half-row at column w / 2 aligned as well)
void plane_wg53(const PlanOptions &o, const PlanSpec &S, const Level &Lv, LevelTables &T) {
    bool ok = true;
    int multi = 0;
    for (size_t i = 0; i < Lv.planes.size() && ok; i++) {
        if (!wg_geometry(Lv.pw[i], Lv.ph[i], true)) ok = false;
        if (Lv.l == 0 && (S.W % 8)) ok = false;                  // packed Gray16 rows: 16-byte lanes of the frame
        if (Lv.pw[i] > 512) multi = 1;
    }
    // Where it pays: a lane takes eight columns, so planes narrower than 512 leave lanes idle -- fine while the
    // level is latency-bound (few waves: the deeper levels of one big plane), a loss against the general
    // kernels' four-columns-per-lane variant when there are many such planes (C2's level 1: 120 planes of
    // 256 x 256, measured 13.1 us against 10.4 us in the inverse)
    if (ok && Lv.maxw < 512) {
        int64_t prows = 0;
        for (size_t i = 0; i < Lv.planes.size(); i++) prows += half(Lv.ph[i]);
        if (prows > 4096) ok = false;
    }
    if (!ok) return;
    for (size_t i = 0; i < Lv.planes.size(); i++)
        for (int c0 = 0; c0 < Lv.pw[i]; c0 += 512) add_bands(T.pjobs, (int)i, 0, half(Lv.ph[i]), o.plane_wg - 1, c0);
    if (o.l0_xcd && T.pjobs.size() >= 64) xcd_chunked(T.pjobs);          // XCD-aware order, as for the RGBA8 kernels
    T.pnjobs = (int)T.pjobs.size(); T.pwaves = o.plane_wg; T.pmulti = multi;
    T.p_pix_only = (Lv.cls == 1 && !o.plane_wg3);
}
// single planes of the 9-7 transform in workgroup form (dwt97_l0wg.inc SRC = 1 / 2, dwt97_l0wg_inv.inc): the deeper
// levels (float64 scratch in, int32 coefficients), and since round 4 level 0 of one int32 component (gray frames,
// frames without the colour transform) and the float64 unit calls (dwt.go:432-473, 551-573): one job per (plane,
// band of NW - 3 pair-rows)
void plane_wg97(const PlanOptions &o, const Level &Lv, LevelTables &T) {
    for (size_t i = 0; i < Lv.planes.size(); i++) {
        const DwtPlane &D = Lv.planes[i];
        if (!wg_geometry(Lv.pw[i], Lv.ph[i]) || !offsets_aligned(D)) return;
        if (Lv.l == 0 && ((D.src_stride % 4) || (D.out_stride % 4))) return;      // a frame's rows: 16-byte row accesses
    }
    const int nr = o.plane_wg97 - 3;
    for (size_t i = 0; i < Lv.planes.size(); i++) add_bands(T.pjobs, (int)i, 0, half(Lv.ph[i]), nr);
    if (o.l0_xcd && T.pjobs.size() >= 64) xcd_dealt(T.pjobs, nr, Lv.ph);
    T.pnjobs = (int)T.pjobs.size(); T.pwaves = o.plane_wg97; T.pmulti = 0;
}

// ------------------------------------------------------------------------------
// level 0 of packed RGBA8 frames (5-3): workgroup tables of both directions, the merged launches, levels 0 + 1 fused
// ------------------------------------------------------------------------------
// first pair-row of plane i that the top bands of nr rows do not cover: the top bands are those that cover the low-pass rows feeding level 1
int split_row(const Level &Lv, size_t i, int nr) {
    const int halfH0 = half(Lv.ph[i]), tb = half(halfH0);
    return std::min(halfH0, ((tb + nr - 1) / nr) * nr);
}
// workgroup form (dwt53_l0pix.inc): one job per workgroup of `waves` waves = waves - 1 pair-rows of one plane
// top_only: just the top bands (the merged launches take the rest)
Jobs rgba8_wg_table(const PlanOptions &o, const Level &Lv, int waves, bool top_only = false, int xcd_group = 0) {
    Jobs wj;
    const int nr = waves - 1;
    for (size_t i = 0; i < Lv.planes.size(); i++) add_bands(wj, (int)i, 0, top_only ? split_row(Lv, i, nr) : half(Lv.ph[i]), nr);
    if (!o.l0_xcd || wj.size() < 64) return wj;
    if (xcd_group > 0) xcd_grouped(wj, (size_t)xcd_group);
    else if (o.l0_deal) xcd_dealt(wj, nr, Lv.ph);
    else xcd_chunked(wj);
    return wj;
}
// merged launches (dwt53_mega_*_kernel): every level below 0 + the level-0 bands that neither feed nor
// need them, for frames of RGB triples only whose deep launch starts at level 1
void merged_launches(const PlanOptions &o, const Level &Lv, int invw, const DeepRoles &R, PlanTables &T) {
    const int order = o.mega;       // 1: deep, level-0 bands, flat; 2: deep, flat, level-0 bands
    for (int d2 = 0; d2 < 2; d2++) {
        const int nr_top = (d2 == 0 ? o.l0_wg : invw) - 1;
        Jobs l0b;
        for (size_t i = 0; i < Lv.planes.size(); i++) add_bands(l0b, (int)i, split_row(Lv, i, nr_top), half(Lv.ph[i]), 15, 2);
        Jobs mj = R.deep[d2];
        const Jobs &fj = R.flat[d2];
        if (order == 2) mj.insert(mj.end(), fj.begin(), fj.end());
        mj.insert(mj.end(), l0b.begin(), l0b.end());
        if (order != 2) mj.insert(mj.end(), fj.begin(), fj.end());
        Jobs top = rgba8_wg_table(o, Lv, nr_top + 1, true, d2 == 1 ? o.l0_xcd_group : 0);
        int64_t top_px = 0;
        for (size_t i = 0; i < Lv.planes.size(); i++) top_px += (int64_t)std::min(2 * split_row(Lv, i, nr_top), Lv.ph[i]) * Lv.pw[i];
        (d2 == 0 ? T.mega_fwd_njobs : T.mega_inv_njobs) = (int)mj.size();
        (d2 == 0 ? T.fwd_top_njobs : T.inv_top_njobs) = (int)top.size();
        (d2 == 0 ? T.fwd_top_bytes : T.inv_top_bytes) = top_px * 16;
        (d2 == 0 ? T.mega_fwd_jobs : T.mega_inv_jobs).swap(mj);
        (d2 == 0 ? T.fwd_top_jobs : T.inv_top_jobs).swap(top);
    }
}
// levels 0 + 1 in one launch (dwt53_fwd_rgba8_wg2_kernel): the bands of the top half of every plane, l0_fuse waves each, and the remaining bands
void fused_level01(const PlanOptions &o, const Level &Lv, PlanTables &T) {
    for (size_t i = 0; i < Lv.planes.size(); i++) {
        const int halfH = half(Lv.ph[i]);
        const int pr = add_bands(T.fwd_wg2_jobs, (int)i, 0, half(halfH), o.l0_fuse - 3);
        add_bands(T.fwd_wg_rest_jobs, (int)i, pr, halfH, o.l0_wg - 1);
    }
    for (Jobs *v : {&T.fwd_wg2_jobs, &T.fwd_wg_rest_jobs})
        if (o.l0_xcd && v->size() >= 64) xcd_chunked(*v);
    T.fwd_wg2_njobs = (int)T.fwd_wg2_jobs.size(); T.fwd_wg2_waves = o.l0_fuse; T.fwd_wg_rest_njobs = (int)T.fwd_wg_rest_jobs.size();
}
// Lv: forward level 0 of the RGB triples, vector accesses, eight columns per lane
void rgba8_level0(const PlanOptions &o, const PlanSpec &S, const Level &Lv, const DeepRoles &R, PlanTables &T) {
    const bool mal = S.mallat;
    if (!mal) {     // (the general kernels have no packed-pixel Mallat instantiation)
        // the packed-pixel forward (j2k_plan_forward_rgba8) moves a third of the bytes per row on the read side
        // and likes shorter bands: its own job table (measured: 3 pair-rows 29.6 us, 5 pair-rows 31.9 us)
        T.fwd_pix_jobs = level_jobs(o, S, Lv, o.band_prows_pix);
        T.fwd_pix_njobs = (int)T.fwd_pix_jobs.size();
    }
    // the workgroup form's geometry contract: one 512-column strip, whole 16-byte lanes, at least two rows
    if (o.l0_wg <= 0) return;
    for (size_t i = 0; i < Lv.planes.size(); i++)
        if (!wg_geometry(Lv.pw[i], Lv.ph[i])) return;
    // one table per direction: the forward kernel measures best with 8 waves per workgroup (7 pair-rows:
    // 3 halo rows per 14), the inverse with 4 (A/B on one box: forward 22.5-23.0 / 21.8-21.9 us at 4 / 8,
    // inverse 25.5 / 26.2)
    // (a Mallat plan: only the shapes its kernels are instantiated for -- forward 8 waves with nt stores, inverse 4 waves
    //  with everything in registers, the defaults; any other setting keeps the general Mallat launch and staged pixels)
    const int invw = o.l0_wg_invw > 0 ? o.l0_wg_invw : o.l0_wg;
    if (!mal || (o.l0_wg == 8 && o.l0_store == 1)) {
        T.fwd_wg_jobs = rgba8_wg_table(o, Lv, o.l0_wg);
        T.fwd_wg_njobs = (int)T.fwd_wg_jobs.size();
        T.fwd_wg_waves = o.l0_wg;
    }
    if (!mal || (invw == 4 && o.l0_inv_wpe == 5)) {
        T.inv_wg_jobs = rgba8_wg_table(o, Lv, invw, false, o.l0_xcd_group);      // (measured: inverse 25.2 -> 24.5 us at groups of 8; the forward table loses 0.5 us with it)
        T.inv_wg_njobs = (int)T.inv_wg_jobs.size();
        T.inv_wg_waves = invw;
    }
    if (!mal && o.mega && T.deep_l0 == 1 && S.C == 3 && Lv.planes.size() == T.groups.size() && !R.deep[0].empty()) merged_launches(o, Lv, invw, R, T);
    // the fused launch needs a level 1 (levels >= 2), only RGB triples in the frame (the level-1 plane table is then three planes per
    // level-0 plane, same order)
    if (!mal && o.l0_fuse > 0 && S.levels >= 2 && S.C == 3 && (T.tail_l0 < 0 || T.tail_l0 >= 2) && (T.deep_l0 < 0 || T.deep_l0 >= 2)) fused_level01(o, Lv, T);
}

// ------------------------------------------------------------------------------
// level 0 of lossy RGB triples in workgroup form (dwt97_l0wg.inc, dwt97_l0wg_inv.inc)
// ------------------------------------------------------------------------------
// forward: one job per (plane, band of NW - 3 pair-rows, component); the three components of a band are neighbours in the table and the
// whole table is dealt XCD-aware like the 5-3 one, so the rows they share are L2 hits; inverse: one job per (plane, band), all three
// components in the workgroup
Jobs l0_wg97_table(const PlanOptions &o, const PlanSpec &S, const Level &Lv, int waves, int ncomp_jobs) {
    Jobs wj;
    if (S.W % 4) return wj;
    for (size_t i = 0; i < Lv.planes.size(); i++)
        if (!wg_geometry(Lv.pw[i], Lv.ph[i]) || !offsets_aligned(Lv.planes[i])) return wj;
    const int nr = waves - 3;
    for (size_t i = 0; i < Lv.planes.size(); i++) add_bands(wj, (int)i, 0, half(Lv.ph[i]), nr, 0, ncomp_jobs);
    if (o.l0_xcd && wj.size() >= 64) xcd_dealt(wj, nr, Lv.ph);
    return wj;
}

// ------------------------------------------------------------------------------
// every level's tables, both directions
// ------------------------------------------------------------------------------
void level_tables(const PlanOptions &o, const PlanSpec &S, const DeepRoles &R, int dir, int l, int cls, PlanTables &T) {
    const bool mal = S.mallat;
    const int esz = S.wavelet == W97 ? 8 : 4;
    Level Lv = level_planes(S, T.groups, dir, l, cls, l == 0, FrameDst{S.W, S.H, 0}, !o.force_novec);
    LevelTables &LT = (dir == 0 ? T.fwd : T.inv)[cls][l];
    LT.ncomp = cls ? 3 : 1;
    LT.mallat = mal;
    LT.nplanes = (int)Lv.planes.size();
    if (Lv.planes.empty()) return;
    level_rule(S, Lv, l == 0 ? S.W : 0, l == 0 ? o.cpl0 : 0, LT);   // (cpl0: tuning knob J2K_CPL0)
    for (size_t i = 0; i < Lv.planes.size(); i++) LT.alg_bytes += (int64_t)2 * esz * Lv.pw[i] * Lv.ph[i] * LT.ncomp;
    LT.jobs = level_jobs(o, S, Lv, general_band(o, S, dir));
    LT.njobs = (int)LT.jobs.size();
    LT.planes = Lv.planes;
    // cls 1 = level 0 of RGB triples: int32 planes (J2K_PLANE_WG3) or RGBA64 pixels
    if ((!mal || l == 0) && S.wavelet == W53 && Lv.vec_ok && o.plane_wg > 0 && (cls == 0 || o.plane_wg3 || l == 0)) plane_wg53(o, S, Lv, LT);
    if (!mal && S.wavelet == W97 && cls == 0 && o.plane_wg97 > 0) plane_wg97(o, Lv, LT);
    if (dir == 0 && l == 0 && cls == 1 && S.wavelet == W53 && Lv.vec_ok && Lv.cpl == 8) rgba8_level0(o, S, Lv, R, T);
    const bool rgb97 = !mal && l == 0 && cls == 1 && S.wavelet == W97 && S.mct && !S.frame_is_f64;
    // (precision <= 16 and Quality < 8192 keep every value the forward kernel converts inside int32: round_half_away_inrange)
    if (rgb97 && dir == 0 && o.l0_wg97 > 0 && S.precision <= 16 && S.quality > 0 && S.quality < 8192) {
        T.fwd97_wg_jobs = l0_wg97_table(o, S, Lv, o.l0_wg97, 3);
        T.fwd97_wg_njobs = (int)T.fwd97_wg_jobs.size();
        if (T.fwd97_wg_njobs) T.fwd97_wg_waves = o.l0_wg97;
    }
    if (rgb97 && dir == 1 && S.quant != Q_NONE && o.l0_wg97_inv > 0) {
        T.inv97_wg_jobs = l0_wg97_table(o, S, Lv, o.l0_wg97_inv, 1);
        T.inv97_wg_njobs = (int)T.inv97_wg_jobs.size();
        if (T.inv97_wg_njobs) T.inv97_wg_waves = o.l0_wg97_inv;
    }
    if (dir == 0) {
        T.dwt_bytes += LT.alg_bytes;
        if (l == 0) T.dwt_level0_bytes += LT.alg_bytes;
    }
}

// ------------------------------------------------------------------------------
// code-block jobs: encoder.go:616-673 per tile, top-left addressing (encoder.go:763-795)
// ------------------------------------------------------------------------------
// (closed-loop mode, j2k_params.closed_loop: the same order, but band b of resolution r is the Mallat rectangle of level
//  numRes-1-r of the plane and its blocks are cut from the band's own origin -- the windows partition the plane)
struct BandRect { int x0, y0, w, h; };
BandRect band_rect(const PlanSpec &S, int numRes, int w, int h, int r, int band) {
    BandRect B{0, 0, 0, 0};
    if (!S.closed_loop) {
        const int64_t scale = (int64_t)1 << std::min(numRes - 1 - r, 40);
        B.w = (int)((w + scale - 1) / scale); B.h = (int)((h + scale - 1) / scale);
        if (r > 0) { B.w = half(B.w); B.h = half(B.h); }
        return B;
    }
    const Dim dl = level_dim(w, h, r == 0 ? numRes - 1 : numRes - 1 - r);
    const int wn = half(dl.w), hn = half(dl.h);
    if (r == 0) { B.w = dl.w; B.h = dl.h; }
    else if (band == J2K_BAND_HL) { B.x0 = wn; B.w = dl.w - wn; B.h = hn; }
    else if (band == J2K_BAND_LH) { B.y0 = hn; B.w = wn; B.h = dl.h - hn; }
    else { B.x0 = wn; B.y0 = hn; B.w = dl.w - wn; B.h = dl.h - hn; }
    return B;
}
void block_jobs(const PlanSpec &S, PlanTables &T) {
    const int numRes = S.num_res_jobs > 0 ? S.num_res_jobs : 6;
    const int cbw = S.cb_w > 0 ? S.cb_w : 64, cbh = S.cb_h > 0 ? S.cb_h : 64;
    std::vector<BlockJob> &bj = T.bjobs;
    int64_t slot = 0, dec = 0;
    size_t gi = 0;
    for (int tl = 0; tl < T.tile_count; tl++) {
        // groups of this tile are contiguous; collect per-component coefficient offsets
        std::vector<int64_t> coff(S.C);
        int w = 0, h = 0;
        for (; gi < T.groups.size() && T.groups[gi].tile == tl; gi++) {
            const Group &g = T.groups[gi];
            for (int k = 0; k < g.nc; k++) coff[g.comp0 + k] = g.coef_off[k];
            w = g.w; h = g.h;
        }
        for (int c = 0; c < S.C; c++)
            for (int r = 0; r < numRes; r++)
                for (int b = 0; b < (r == 0 ? 1 : 3); b++) {
                    const int band = r == 0 ? J2K_BAND_LL : (b == 0 ? J2K_BAND_HL : (b == 1 ? J2K_BAND_LH : J2K_BAND_HH));
                    const BandRect B = band_rect(S, numRes, w, h, r, band);
                    for (int cby = 0; cby * cbh < B.h; cby++)
                        for (int cbx = 0; cbx * cbw < B.w; cbx++) {
                            const int sx = B.x0 + cbx * cbw, sy = B.y0 + cby * cbh;
                            const int aw = std::min(cbw, B.w - cbx * cbw), ah = std::min(cbh, B.h - cby * cbh);
                            T.blocks.push_back(j2k_block{tl * S.C + c, band, sx, sy, aw, ah});
                            T.block_tile.push_back(tl);
                            T.block_res.push_back(r);
                            T.max_block_h = std::max(T.max_block_h, ah);
                            T.slot_off.push_back((uint64_t)slot);
                            T.dec_off.push_back((uint64_t)dec);
                            BlockJob J{};
                            J.src_off = coff[c] + (int64_t)sy * w + sx;
                            J.out_off = slot;
                            J.stride = w; J.w = aw; J.h = ah; J.band = band;
                            bj.push_back(J);
                            slot += (int64_t)((j2k_block_bound(S.coder, aw, ah) + 15) & ~size_t(15));
                            dec += align4((int64_t)aw * ah);
                            T.block_samples += (int64_t)aw * ah;
                        }
                }
    }
    T.bytes_cap = slot; T.decoded_elems = dec;
    // first job of every tile of the shard (jobs are enumerated tile by tile) and the largest tile's slot bytes
    std::vector<uint64_t> tstart;
    for (size_t i = 0; i < bj.size(); i++)
        if (i == 0 || T.block_tile[i] != T.block_tile[i - 1]) { T.tile_job0.push_back((int)i); tstart.push_back(T.slot_off[i]); }
    T.tile_job0.push_back((int)bj.size()); tstart.push_back((uint64_t)slot);
    for (size_t t = 0; t + 1 < tstart.size(); t++) T.max_tile_bytes = std::max(T.max_tile_bytes, tstart[t + 1] - tstart[t]);
    // decode table: dense decoded blocks
    T.djobs = bj;
    for (size_t i = 0; i < bj.size(); i++) T.djobs[i].out_off = (int64_t)T.dec_off[i];
    if (S.closed_loop && S.coder == J2K_CODER_HT) {
        // closed-loop HT plans: the frame decoder writes every block straight into its window of the coefficient planes (ht_decode_kernel<true>)
        T.djobs_placed = bj;
        for (BlockJob &J : T.djobs_placed) J.out_off = J.src_off;
    }
}

typedef std::tuple<int64_t, int32_t, int32_t, int32_t> Window;
Window window_of(const BlockJob &J) { return std::make_tuple(J.src_off, J.stride, J.w, J.h); }

// Jobs with the same window are byte-identical for the HT coder (top-left addressing + a coder that ignores the
// band: see ht_encode_kernel): one coded job per distinct window, the others chained to it and gathering from its
// slot.  Only j2k_plan_encode_stream uses these tables (its slot buffer is private); the per-slot API does not.
void ht_alias_tables(PlanTables &T) {
    const std::vector<BlockJob> &bj = T.bjobs;
    std::map<Window, int> first;
    std::vector<int> ujobs;
    std::vector<std::vector<int>> lists;
    std::vector<BlockJob> aj = bj;
    for (size_t i = 0; i < bj.size(); i++) {
        auto it = first.find(window_of(bj[i]));
        if (it == first.end()) { first[window_of(bj[i])] = (int)ujobs.size(); ujobs.push_back((int)i); lists.push_back({(int)i}); }
        else { lists[it->second].push_back((int)i); aj[i].out_off = bj[ujobs[it->second]].out_off; }
    }
    if (ujobs.size() >= bj.size()) return;
    for (size_t u = 0; u < ujobs.size(); u++) {
        T.ht_ujobs.push_back(HtUJob{bj[ujobs[u]], ujobs[u], (int)T.ht_alias_next.size(), (int)lists[u].size(), 0});
        T.ht_alias_next.insert(T.ht_alias_next.end(), lists[u].begin(), lists[u].end());
    }
    T.ht_nunique = (int)ujobs.size();
    T.bjobs_alias.swap(aj);
}

// The same fact for the decoder (option ht_dec_dedup; whatever ht_alias says): jobs with the same window carry the same bytes in any
// stream this encoder wrote, so one decode can serve them all.  These tables only NAME candidates -- ht_vlcprep_kernel compares the
// bytes of every call's stream and a job that differs decodes itself.  Leader = the lowest job of the window.  A job follows it only
// on static facts of the pair: same w and h, a lean width (8, 16, 32, 64), the geometry on the parallel path (ht_vlc_head's `fast`),
// both decoded blocks 16-byte aligned (ht_decode_lean_kernel's own condition), and the leader's list not yet full.
void ht_decode_tables(const PlanLimits &lim, PlanTables &T) {
    const std::vector<BlockJob> &bj = T.bjobs;
    const size_t nj = bj.size();
    std::map<Window, int> lead;
    T.ht_dec_rep.resize(nj);
    std::vector<int32_t> fol(nj * (size_t)(J2K_HT_DEC_MAX_FOLLOWERS + 1), 0);
    for (size_t i = 0; i < nj; i++) {
        T.ht_dec_rep[i] = (int32_t)i;
        auto ins = lead.emplace(window_of(bj[i]), (int)i);
        if (ins.second) continue;
        const int L = ins.first->second, w = bj[i].w, h = bj[i].h;
        const int R = (h + 3) / 4, Np = R * (((w + 3) / 4 + 1) / 2);
        const bool fast = (size_t)R * (size_t)w <= (size_t)lim.ht_fast_max_samples && Np <= lim.ht_walk_max_pairs;
        int32_t *row = &fol[(size_t)L * (J2K_HT_DEC_MAX_FOLLOWERS + 1)];
        if (bj[L].w != w || bj[L].h != h || !(w == 8 || w == 16 || w == 32 || w == 64) || !fast) continue;
        if ((T.dec_off[i] & 3) || (T.dec_off[L] & 3) || row[0] >= J2K_HT_DEC_MAX_FOLLOWERS) continue;
        row[++row[0]] = (int32_t)i;
        T.ht_dec_rep[i] = L;
        T.ht_dec_any = true;
    }
    // The walk's order (ht_walk_kernel<true>): one block per lane, and only a job that is its own leader is sure to walk -- those first, ascending,
    // so that they fill whole workgroups; the static followers behind them, in workgroups that leave at once when every follower verifies.
    for (size_t i = 0; i < nj; i++) if (T.ht_dec_rep[i] == (int32_t)i) T.ht_walk_order.push_back((int32_t)i);
    T.ht_walk_nlead = (int)T.ht_walk_order.size();
    for (size_t i = 0; i < nj; i++) if (T.ht_dec_rep[i] != (int32_t)i) T.ht_walk_order.push_back((int32_t)i);
    if (!T.ht_dec_any) return;
    T.ht_walk_pos.resize(nj);
    for (size_t s = 0; s < nj; s++) T.ht_walk_pos[(size_t)T.ht_walk_order[s]] = (int32_t)s;
    T.ht_dec_fol.swap(fol);
}

// The 16-bit hand-off of X_1 (option l0_scr16): only where the writer is the packed-RGBA8 workgroup kernel in its default shape (eight
// waves, nt stores -- the one instantiation of dwt53_fwd_rgba8_wg16_kernel) and the only reader the deep launch starting at level 1.
// Everything else keeps int32 rows: Mallat plans, 9-7, level 0 fused with level 1 (l0_fuse) or merged with the deep launch (mega), frames
// with a single-component plane beside the triples (the plane kernels write its prefix), the per-level and LDS-tail launches.  The
// planar calls of the same plan (arbitrary int32 planes) and a YCbCr source keep int32 rows in the same buffer: the choice is made per
// call (plan_forward_impl), the row slots are the same.  8-bit unsigned samples bound what is stored (J2K_SCR16_BOUND).
void scr16_forms(const PlanOptions &o, const PlanSpec &S, PlanTables &T) {
    const bool deep_rgb = S.wavelet == W53 && !S.mallat && S.C == 3 && S.mct && T.deep_l0 == 1;
    T.scr16_fwd = (o.l0_scr16 & 1) && deep_rgb && S.precision == 8 && S.dc_shift == 128 && J2K_SCR16_BOUND + S.dc_shift <= INT16_MAX &&
                  !T.deep_jobs.empty() && !T.fwd_wg_jobs.empty() && T.fwd_wg_waves == 8 &&
                  T.fwd_wg2_jobs.empty() && T.mega_fwd_jobs.empty() && !T.fwd[0][0].njobs;      // (and l0_store == 1, read per call as the launch reads it)
    // The inverse direction (option bit 1): the values are a decoder's, so the format is chosen per stored row at run time (dwt53_deep_inv_body's
    // vote) and recorded in d_scr16_fmt, one byte per 8 elements of the scratch (rows of X_1 are at least 8 long), rewritten by every call that
    // uses it.  Only where the one reader of X_1 is the packed-RGBA8 workgroup kernel in its default shape (four waves, everything in registers
    // -- the one instantiation of dwt53_inv_rgba8_wg16_kernel), per call (plan_inverse_impl): the general level-0 kernel (planar, reduced and
    // area calls, l0_wg_inv = 0), the plane kernels (a fourth component: no such plane may be in the frame) and the merged launch read int32 rows
    // and get them from dwt53_deep_inv_kernel as ever.  Batch and shard plans are plans like any other here: same tables, same two launches.
    T.scr16_inv = (o.l0_scr16 & 2) && deep_rgb && !T.deep_jobs_inv.empty() && !T.inv_wg_jobs.empty() && T.inv_wg_waves == 4 && !T.inv[0][0].njobs &&
                  T.scrA_elems;
}

}  // namespace

namespace j2k {

int build_plan_tables(const PlanOptions &o, const PlanLimits &lim, const PlanSpec &S, PlanTables &T, const char **why) {
    if (S.W <= 0 || S.H <= 0 || S.C <= 0 || S.levels < 0 || S.levels > 32) { *why = "bad geometry"; return J2K_ERR_INVALID_ARG; }
    if ((int64_t)S.W * S.H >= (int64_t)1 << 31) { *why = "plane too large"; return J2K_ERR_INVALID_ARG; }
    T = PlanTables();
    const int L = S.levels;
    // a Mallat plan: the MAL kernels for every level, one general launch each.  Of the specialised 5-3 forms it has the two that read / write
    // packed pixels at level 0 -- the RGBA8 workgroup tables (the shapes the launchers have a MAL instantiation for) and the plane-workgroup
    // table of level 0; not the tail / deep / mega / fused-level launches, not the plane-workgroup form below level 0 (measured: they did not pay,
    // docs/KERNEL_NOTES.md "§4r, continued"), nothing 9-7
    const bool lds_forms = S.wavelet == W53 && !S.mallat;
    tile_components(S, T);
    if (lds_forms && o.use_tail && L >= 3) lds_tail(S, T);
    DeepRoles R;
    const int lds_l0 = lds_forms ? first_lds_level(T.groups, L - 1) : -1;      // (the tail above needs two such levels, the deep launch one)
    if (lds_l0 >= 2 && o.use_deep) deep_launch(o, S, lds_l0, T, R);
    for (int cls = 0; cls < 2; cls++) { T.fwd[cls].resize(L); T.inv[cls].resize(L); }
    for (int dir = 0; dir < 2; dir++)
        for (int l = 0; l < L; l++)
            for (int cls = 0; cls < 2; cls++) level_tables(o, S, R, dir, l, cls, T);
    block_jobs(S, T);
    if (S.coder == J2K_CODER_HT && o.ht_alias) ht_alias_tables(T);
    if (S.coder == J2K_CODER_HT) ht_decode_tables(lim, T);
    scr16_forms(o, S, T);
    return J2K_OK;
}

// ------------------------------------------------------------------------------
// Mallat plans, reduced-resolution decode: the tables of one `reduce`
// ------------------------------------------------------------------------------
int check_reduce(const PlanSpec &S, int reduce, const char **why) {
    if (!S.mallat) { *why = "reduced-resolution decode needs a Mallat plan (j2k_params.closed_loop = J2K_CLOSED_LOOP_MALLAT): no other plan's coarser levels are pictures"; return J2K_ERR_UNSUPPORTED; }
    if (reduce < 0 || reduce > S.levels) { *why = "reduce outside 0 ... decomposition levels"; return J2K_ERR_INVALID_ARG; }
    const int fh = S.frame_h > 0 ? S.frame_h : S.H;
    const int tw = S.tile_w > 0 ? S.tile_w : S.W, th = S.tile_h > 0 ? S.tile_h : fh;
    const int mask = (int)(((int64_t)1 << reduce) - 1);
    // a tile's origin must stay a whole sample of the reduced frame, or the reduced tiles would overlap or leave gaps
    if ((tw < S.W && (tw & mask)) || (th < fh && (th & mask))) { *why = "reduce: the tile size is not a multiple of 2^reduce"; return J2K_ERR_INVALID_ARG; }
    if (fh < S.H && (fh & mask)) { *why = "reduce: frame_rows is not a multiple of 2^reduce"; return J2K_ERR_INVALID_ARG; }
    return J2K_OK;
}

int build_reduced_tables(const PlanOptions &o, const PlanSpec &S, const PlanScalars &P, int reduce, ReducedTables &R, const char **why) {
    const int r = check_reduce(S, reduce, why);
    if (r != J2K_OK) return r;
    const int L = S.levels, mask = (int)(((int64_t)1 << reduce) - 1);
    R = ReducedTables();
    if (reduce == 0) return J2K_OK;      // exactly the call without it: nothing is built
    auto shr = [&](int v) { return (int)(((int64_t)v + mask) >> reduce); };      // ceil(v / 2^reduce) = `reduce` times (v + 1) / 2
    R.Wr = shr(S.W); R.Hr = shr(S.H);
    const FrameDst F{R.Wr, R.Hr, reduce};
    if (reduce == L) {      // no level runs: the LL rectangles are the picture
        const Level Lv = level_planes(S, P.groups, 1, reduce, -1, true, F, true);
        for (size_t i = 0; i < Lv.planes.size(); i++) {
            const DwtPlane &D = Lv.planes[i];
            LLPlane Q{};
            for (int k = 0; k < 3; k++) { Q.coef_off[k] = D.src_off[k]; Q.out_off[k] = D.out_off[k]; }
            Q.w = D.w; Q.h = D.h; Q.coef_stride = D.coef_stride; Q.out_stride = D.out_stride; Q.nc = Lv.pnc[i];
            R.ll_samples = std::max(R.ll_samples, Q.w * Q.h);
            R.ll.push_back(Q);
        }
        R.nll = (int)R.ll.size();
    } else {
        // level `reduce` as the final launch: its planes grouped as MCT triples, as level 0 groups them; the general kernels, unlinked bands
        for (int cls = 0; cls < 2; cls++) {
            Level Lv = level_planes(S, P.groups, 1, reduce, cls, true, F, !o.force_novec);
            LevelTables &T = R.inv[cls];
            T.ncomp = cls ? 3 : 1; T.mallat = true; T.nplanes = (int)Lv.planes.size();
            if (Lv.planes.empty()) continue;
            level_rule(S, Lv, R.Wr, 0, T);
            T.jobs = general_jobs(Lv, general_band(o, S, 1));
            T.njobs = (int)T.jobs.size();
            T.planes = Lv.planes;
        }
    }
    // the code-block jobs a decode to this resolution needs: resolutions 0 ... num_resolutions - 1 - reduce
    const int numRes = S.num_res_jobs > 0 ? S.num_res_jobs : 6;
    for (size_t j = 0; j < P.blocks.size(); j++) {
        if (P.block_res[j] > numRes - 1 - reduce) continue;
        const j2k_block &b = P.blocks[j];
        const int64_t *d = &P.plane_desc[(size_t)b.plane * 7];      // tile, comp, x0, y0, w, h, coefficient offset
        BlockJob J{};
        J.src_off = d[6] + (int64_t)b.y0 * d[4] + b.x0;
        J.stride = (int32_t)d[4]; J.w = b.w; J.h = b.h; J.band = b.band;
        J.out_off = (int64_t)P.slot_off[j]; R.bjobs.push_back(J);
        J.out_off = (int64_t)P.dec_off[j]; R.djobs.push_back(J);
        J.out_off = J.src_off;
        if (S.coder == J2K_CODER_HT) R.placed.push_back(J);
        R.ids.push_back((int)j);
        R.max_block_h = std::max(R.max_block_h, b.h);
    }
    R.njobs = (int)R.ids.size();
    return J2K_OK;
}

}  // namespace j2k

// ------------------------------------------------------------------------------
// frames of a batch as job ranges (the rate allocation of j2k_plan_set_rate_per_frame)
// ------------------------------------------------------------------------------
namespace j2k {
bool frame_job_ranges(const std::vector<int32_t> &block_tile, int tiles_per_frame, int nframes, std::vector<RateFrame> &out) {
    out.clear();
    if (tiles_per_frame < 1 || nframes < 1) return false;
    const size_t n = block_tile.size();
    size_t j = 0;
    for (int f = 0; f < nframes; f++) {
        const int64_t t0 = (int64_t)f * tiles_per_frame, t1 = t0 + tiles_per_frame;
        const size_t first = j;
        while (j < n && block_tile[j] >= t0 && block_tile[j] < t1) j++;
        out.push_back(RateFrame{(int32_t)first, (int32_t)(j - first)});
    }
    if (j != n) { out.clear(); return false; }       // a tile out of order or out of range: the jobs of a frame would not be one range
    return true;
}
}  // namespace j2k
