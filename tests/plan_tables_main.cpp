// plan_tables_main.cpp -- a stand-alone driver of the plan's table builder (go-jpeg2000_amd/csrc/plan_tables.h: no HIP in it), built with
// AddressSanitizer + UBSan by tests/test_plan_tables.py and run directly.  For every case of a fixed matrix of geometries and option settings it
//   * prints every table build_plan_tables makes (element size : count : FNV-1a 64 of its bytes) and every scalar it derives, keyed by name, and
//     for Mallat plans the tables of every valid `reduce` -- the test compares that with tests/plan_tables_recorded.json, which was recorded from
//     the builder as it was before it left j2k_planbuild.cpp;
//   * checks what every band table must hold whatever its order: planes exist, the bands of every (plane, column strip) own every pair-row exactly
//     once, link flags come as pairs inside a workgroup's four jobs, padding is {-1, 0, 0, 0}; block windows lie in their planes, slots and
//     decoded blocks do not overlap.  A violation is printed and the exit status is 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "../go-jpeg2000_amd/csrc/plan_tables.h"

using namespace j2k;

static int g_bad = 0;
static std::string g_run;
static void bad(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "INVARIANT %s: ", g_run.c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    g_bad++;
}

// ---- output: "name value" lines ------------------------------------------------------------------------------------------------------------
static uint64_t fnv1a(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <class E>
static void table(const std::string &name, const std::vector<E> &v, bool always = true) {
    if (v.empty()) { if (always) printf("%s %zu:0:-\n", name.c_str(), sizeof(E)); return; }
    printf("%s %zu:%zu:%016llx\n", name.c_str(), sizeof(E), v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(E)));
}
static void table_groups(const std::string &name, const std::vector<Group> &v) {      // (Group has padding: its fields, not its bytes)
    uint64_t h = fnv1a("", 0);
    for (const Group &g : v) {
        const int32_t a[7] = {g.tile, g.comp0, g.nc, g.x0, g.y0, g.w, g.h};
        h = fnv1a(a, sizeof(a), h); h = fnv1a(g.coef_off, 24, h); h = fnv1a(g.scrA_off, 24, h); h = fnv1a(g.scrB_off, 24, h);
    }
    printf("%s 100:%zu:%016llx\n", name.c_str(), v.size(), (unsigned long long)h);
}
static void scalars(const std::string &name, std::initializer_list<long long> v) {
    printf("%s ", name.c_str());
    const char *sep = "";
    for (long long x : v) { printf("%s%lld", sep, x); sep = ","; }
    printf("\n");
}
static void level(const std::string &name, const LevelTables &T) {
    scalars(name + ".info", {T.njobs, T.nplanes, T.cpl, T.vec, T.ncomp, T.alg_bytes, T.pnjobs, T.pwaves, T.pmulti, T.p_pix_only, T.mallat});
    table(name + ".planes", T.planes, false); table(name + ".jobs", T.jobs, false); table(name + ".pjobs", T.pjobs, false);
}
static std::string idx(const char *what, int a, int b = -1) {
    char buf[64];
    if (b >= 0) snprintf(buf, sizeof(buf), "%s[%d][%d]", what, a, b); else snprintf(buf, sizeof(buf), "%s[%d]", what, a);
    return buf;
}

static void dump_plan(const PlanTables &T) {
    scalars("s.tiles", {T.tiles_x, T.tiles_y, T.tile_first, T.tile_count});
    scalars("s.elems", {T.coeff_elems, T.scrA_elems, T.scrB_elems});
    scalars("s.tail", {T.tail_l0, T.ntail, (long long)T.tail_lds_fwd, (long long)T.tail_lds_inv});
    scalars("s.deep", {T.deep_l0, T.ndeep_jobs, T.ndeep_jobs_inv, (long long)T.deep_lds, (long long)T.deep_lds_fwd});
    scalars("s.scr16", {T.scr16_fwd, T.scr16_inv});
    scalars("s.mega", {T.mega_fwd_njobs, T.mega_inv_njobs, T.fwd_top_njobs, T.inv_top_njobs, T.fwd_top_bytes, T.inv_top_bytes});
    scalars("s.blocks", {T.max_block_h, (long long)T.max_tile_bytes, T.bytes_cap, T.decoded_elems, T.block_samples});
    scalars("s.dwt_bytes", {T.dwt_bytes, T.dwt_level0_bytes});
    scalars("s.ht", {T.ht_nunique, T.ht_walk_nlead});
    scalars("s.wg", {T.fwd_pix_njobs, T.fwd_wg_njobs, T.fwd_wg_waves, T.inv_wg_njobs, T.inv_wg_waves, T.fwd_wg2_njobs, T.fwd_wg2_waves, T.fwd_wg_rest_njobs});
    scalars("s.wg97", {T.fwd97_wg_njobs, T.fwd97_wg_waves, T.inv97_wg_njobs, T.inv97_wg_waves});
    table_groups("host.groups", T.groups);
    table("host.plane_desc", T.plane_desc); table("host.blocks", T.blocks); table("host.block_tile", T.block_tile); table("host.block_res", T.block_res);
    table("host.slot_off", T.slot_off); table("host.dec_off", T.dec_off); table("host.ht_dec_rep", T.ht_dec_rep); table("host.ht_walk_order", T.ht_walk_order);
    for (int cls = 0; cls < 2; cls++)
        for (size_t l = 0; l < T.fwd[cls].size(); l++) { level(idx("fwd", cls, (int)l), T.fwd[cls][l]); level(idx("inv", cls, (int)l), T.inv[cls][l]); }
    table("tail", T.tail); table("deep_planes", T.deep_planes); table("deep_jobs", T.deep_jobs); table("deep_jobs_inv", T.deep_jobs_inv);
    table("mega_fwd_jobs", T.mega_fwd_jobs); table("mega_inv_jobs", T.mega_inv_jobs); table("fwd_top_jobs", T.fwd_top_jobs); table("inv_top_jobs", T.inv_top_jobs);
    table("fwd_pix_jobs", T.fwd_pix_jobs); table("fwd_wg_jobs", T.fwd_wg_jobs); table("inv_wg_jobs", T.inv_wg_jobs);
    table("fwd_wg2_jobs", T.fwd_wg2_jobs); table("fwd_wg_rest_jobs", T.fwd_wg_rest_jobs); table("fwd97_wg_jobs", T.fwd97_wg_jobs); table("inv97_wg_jobs", T.inv97_wg_jobs);
    table("tile_job0", T.tile_job0); table("bjobs", T.bjobs); table("djobs", T.djobs); table("djobs_placed", T.djobs_placed);
    table("ht_ujobs", T.ht_ujobs); table("ht_alias_next", T.ht_alias_next); table("bjobs_alias", T.bjobs_alias);
    // (the two device tables that are the host's lists, uploaded only when some job has a follower)
    static const std::vector<int32_t> none;
    table("ht_dec_rep", T.ht_dec_any ? T.ht_dec_rep : none); table("ht_dec_fol", T.ht_dec_fol);
    table("ht_walk_order", T.ht_dec_any ? T.ht_walk_order : none); table("ht_walk_pos", T.ht_walk_pos);
}
static void dump_reduced(int reduce, const ReducedTables &R) {
    const std::string n = idx("reduce", reduce);
    scalars(n + ".info", {R.Wr, R.Hr, R.nll, R.ll_samples, R.njobs, R.max_block_h});
    for (int cls = 0; cls < 2; cls++) level(n + idx(".inv", cls), R.inv[cls]);
    table(n + ".ll", R.ll, false); table(n + ".ids", R.ids, false); table(n + ".bjobs", R.bjobs, false); table(n + ".djobs", R.djobs, false);
    table(n + ".placed", R.placed, false);
}

// ---- invariants ----------------------------------------------------------------------------------------------------------------------------
typedef std::vector<DwtJob> Jobs;
// Every entry of `tabs` names a plane of `planes` or is padding; the bands of every (plane, col0) own each pair-row of the plane exactly once
// (top_only: each at most once, a prefix that covers the rows feeding the next level); `links`: the table may carry J2K_LINK_* flags.
static void check_bands(const char *what, const std::vector<DwtPlane> &planes, std::initializer_list<const Jobs *> tabs, bool links = false, bool top_only = false) {
    std::map<std::pair<int, int>, std::vector<int>> owned;
    std::vector<int> seen(planes.size(), 0);
    for (const Jobs *jp : tabs) {
        const Jobs &J = *jp;
        for (size_t i = 0; i < J.size(); i++) {
            const DwtJob &j = J[i];
            if (j.plane < 0) {
                if (j.plane != -1 || j.col0 || j.prow0 || j.nprow) bad("%s[%zu]: padding is not {-1, 0, 0, 0}", what, i);
                continue;
            }
            if ((size_t)j.plane >= planes.size()) { bad("%s[%zu]: plane %d of %zu", what, i, j.plane, planes.size()); continue; }
            const int halfH = std::max((planes[j.plane].h + 1) / 2, 1), n = j.nprow & 0xffff, flags = j.nprow & ~0xffff;
            seen[j.plane] = 1;
            if (n <= 0 || j.prow0 < 0 || j.prow0 >= halfH) bad("%s[%zu]: band %d + %d of %d pair-rows", what, i, j.prow0, n, halfH);
            std::vector<int> &o = owned[{j.plane, j.col0}];
            o.resize(halfH, 0);
            for (int r = j.prow0; r < std::min(j.prow0 + n, halfH); r++) o[r]++;
            if (flags && !links) bad("%s[%zu]: flags 0x%x in a table that has none", what, i, flags);
            if (flags & ~(J2K_LINK_UP | J2K_LINK_DOWN)) bad("%s[%zu]: unknown flags 0x%x", what, i, flags);
            if (flags & J2K_LINK_DOWN) {
                const bool ok = i % 4 != 3 && i + 1 < J.size() && (J[i + 1].nprow & J2K_LINK_UP) && J[i + 1].plane == j.plane && J[i + 1].col0 == j.col0 && J[i + 1].prow0 == j.prow0 + n;
                if (!ok) bad("%s[%zu]: LINK_DOWN without its LINK_UP neighbour below", what, i);
            }
            if (flags & J2K_LINK_UP) {
                const bool ok = i % 4 != 0 && (J[i - 1].nprow & J2K_LINK_DOWN) && J[i - 1].plane == j.plane && J[i - 1].col0 == j.col0;
                if (!ok) bad("%s[%zu]: LINK_UP without its LINK_DOWN neighbour above", what, i);
            }
        }
    }
    for (size_t p = 0; p < planes.size(); p++) if (!seen[p]) bad("%s: plane %zu has no band", what, p);
    for (const auto &kv : owned) {
        const std::vector<int> &o = kv.second;
        size_t covered = 0;
        while (covered < o.size() && o[covered] == 1) covered++;
        for (size_t r = covered; r < o.size(); r++)
            if (o[r] != 0 || !top_only) { bad("%s: plane %d strip %d pair-row %zu owned %d times", what, kv.first.first, kv.first.second, r, o[r]); break; }
        if (top_only && covered < (o.size() + 1) / 2) bad("%s: plane %d: the top bands stop at pair-row %zu of %zu", what, kv.first.first, covered, o.size());
    }
}
static void check_level(const std::string &name, const LevelTables &T, bool links) {
    if (!T.jobs.empty()) check_bands((name + ".jobs").c_str(), T.planes, {&T.jobs}, links);
    if (!T.pjobs.empty()) check_bands((name + ".pjobs").c_str(), T.planes, {&T.pjobs});
}
static void check_plan(const PlanSpec &S, const PlanTables &T) {
    static const std::vector<DwtPlane> none;
    for (int cls = 0; cls < 2; cls++)
        for (size_t l = 0; l < T.fwd[cls].size(); l++) { check_level(idx("fwd", cls, (int)l), T.fwd[cls][l], true); check_level(idx("inv", cls, (int)l), T.inv[cls][l], true); }
    const std::vector<DwtPlane> &f0 = T.fwd[1].empty() ? none : T.fwd[1][0].planes, &i0 = T.inv[1].empty() ? none : T.inv[1][0].planes;
    if (!T.fwd_pix_jobs.empty()) check_bands("fwd_pix_jobs", f0, {&T.fwd_pix_jobs}, true);
    if (!T.fwd_wg_jobs.empty()) check_bands("fwd_wg_jobs", f0, {&T.fwd_wg_jobs});
    if (!T.inv_wg_jobs.empty()) check_bands("inv_wg_jobs", i0, {&T.inv_wg_jobs});
    if (!T.fwd_top_jobs.empty()) check_bands("fwd_top_jobs", f0, {&T.fwd_top_jobs}, false, true);
    if (!T.inv_top_jobs.empty()) check_bands("inv_top_jobs", i0, {&T.inv_top_jobs}, false, true);
    if (!T.fwd_wg2_jobs.empty()) check_bands("fwd_wg2_jobs + fwd_wg_rest_jobs", f0, {&T.fwd_wg2_jobs, &T.fwd_wg_rest_jobs});
    if (!T.fwd97_wg_jobs.empty()) {
        check_bands("fwd97_wg_jobs", f0, {&T.fwd97_wg_jobs});      // (col0 = the component: each of the three partitions the plane)
        std::vector<int> ncol(f0.size(), 0);
        for (const DwtJob &j : T.fwd97_wg_jobs) if (j.plane >= 0 && (size_t)j.plane < f0.size() && j.prow0 == 0) ncol[j.plane] |= 1 << j.col0;
        for (size_t p = 0; p < f0.size(); p++) if (ncol[p] != 7) bad("fwd97_wg_jobs: plane %zu has components 0x%x", p, ncol[p]);
    }
    if (!T.inv97_wg_jobs.empty()) check_bands("inv97_wg_jobs", i0, {&T.inv97_wg_jobs});
    // block jobs
    const size_t n = T.bjobs.size();
    if (T.blocks.size() != n || T.djobs.size() != n || T.slot_off.size() != n || T.dec_off.size() != n) { bad("block tables of different lengths"); return; }
    for (size_t j = 0; j < n; j++) {
        const j2k_block &b = T.blocks[j];
        const BlockJob &J = T.bjobs[j];
        if (b.plane < 0 || (size_t)b.plane * 7 + 6 >= T.plane_desc.size()) { bad("block %zu: plane %d", j, b.plane); continue; }
        const int64_t *d = &T.plane_desc[(size_t)b.plane * 7];
        if (b.x0 < 0 || b.y0 < 0 || b.w <= 0 || b.h <= 0 || b.x0 + (int64_t)b.w > d[4] || b.y0 + (int64_t)b.h > d[5]) bad("block %zu: window outside its %lld x %lld plane", j, (long long)d[4], (long long)d[5]);
        if (J.src_off != d[6] + (int64_t)b.y0 * d[4] + b.x0 || J.stride != d[4] || J.w != b.w || J.h != b.h) bad("block %zu: job and block disagree", j);
        if (J.out_off != (int64_t)T.slot_off[j] || T.djobs[j].out_off != (int64_t)T.dec_off[j]) bad("block %zu: out_off is not its slot / decoded offset", j);
        const uint64_t slot_end = T.slot_off[j] + j2k_block_bound(S.coder, b.w, b.h), dec_end = T.dec_off[j] + (uint64_t)b.w * b.h;
        if (slot_end > (j + 1 < n ? T.slot_off[j + 1] : (uint64_t)T.bytes_cap)) bad("block %zu: slot overlaps the next", j);
        if (dec_end > (j + 1 < n ? T.dec_off[j + 1] : (uint64_t)T.decoded_elems)) bad("block %zu: decoded block overlaps the next", j);
    }
}

// ---- the matrix ----------------------------------------------------------------------------------------------------------------------------
// j2k_params -> PlanSpec as j2k_plan_create makes it
static PlanSpec frame_spec(int W, int H, int C, int precision, bool lossless, int tile_w, int tile_h, int num_res, int cb, int coder, int closed_loop = 0, int quality = 0) {
    PlanSpec S;
    S.W = W; S.H = H; S.C = C; S.frame_h = H;
    S.tile_w = tile_w; S.tile_h = tile_h;
    S.levels = num_res - 1;
    if (S.levels <= 0) S.levels = 5;
    S.wavelet = lossless ? W53 : W97;
    S.precision = precision;
    S.dc_shift = (int)((uint32_t)1 << (precision - 1));
    S.dc_shift_inv = S.dc_shift;
    S.mct = C >= 3;
    S.quant = lossless ? Q_NONE : Q_ENCODER;
    S.quality = quality > 0 ? quality : 100;
    S.num_res_jobs = num_res > 0 ? num_res : 6;
    S.cb_w = S.cb_h = cb > 0 ? cb : 64;
    S.coder = coder;
    S.closed_loop = closed_loop != 0;
    S.mallat = closed_loop == J2K_CLOSED_LOOP_MALLAT;
    return S;
}
// ... as the unit calls make it (j2k_hostcalls.cpp host_dwt)
static PlanSpec unit_spec(int w, int h, int levels, int wavelet, int quant, bool f64) {
    PlanSpec S;
    S.W = w; S.H = h; S.C = 1; S.levels = levels; S.wavelet = wavelet; S.dc_shift = 0; S.dc_shift_inv = 0; S.mct = 0;
    S.quant = quant; S.frame_is_f64 = f64; S.num_res_jobs = 1; S.cb_w = 1 << 20; S.cb_h = 1 << 20;
    return S;
}

static void run(const std::string &name, const PlanOptions &o, const PlanSpec &S) {
    g_run = name;
    printf("@ %s\n", name.c_str());
    PlanTables T;
    const char *why = "";
    const PlanLimits lim{1024, 128};      // ht.hip: HT_FAST_MAX_SAMPLES, HT_WALK_MAX_PAIRS
    const int r = build_plan_tables(o, lim, S, T, &why);
    if (r != J2K_OK) { printf("refused %d %s\n", r, why); return; }
    dump_plan(T);
    check_plan(S, T);
    for (int reduce = 1; S.mallat && reduce <= S.levels; reduce++) {
        ReducedTables R;
        if (build_reduced_tables(o, S, T, reduce, R, &why) != J2K_OK) continue;
        dump_reduced(reduce, R);
        for (int cls = 0; cls < 2; cls++) check_level(idx("reduce", reduce) + idx(".inv", cls), R.inv[cls], false);
    }
}

struct Option { const char *name; std::function<void(PlanOptions &, long)> set; std::vector<long> values; };
#define OPT(field, ...) Option{#field, [](PlanOptions &o, long v) { o.field = (decltype(o.field))v; }, {__VA_ARGS__}}
// every plan-shaping option at every other value j2k_ctx_set_option takes for it (the open ranges: a value on either side of what they gate)
static const std::vector<Option> &options() {
    static const std::vector<Option> O = {
        OPT(fwd_link, 0), OPT(inv_link, 0), OPT(plane_wg3, 1), OPT(plane_wg, 0, 8), OPT(l0_fuse, 8, 10, 16), OPT(l0_wg, 0, 4), OPT(l0_wg_invw, 0, 8), OPT(l0_deal, 0),
        OPT(l0_wg97, 0, 6, 10, 12, 14, 16), OPT(plane_wg97, 0), OPT(l0_wg97_inv, 0, 6, 10, 12), OPT(l0_xcd_group, 0, 8), OPT(l0_xcd, 0), OPT(ht_alias, 0),
        OPT(l0_inv_wpe, 6, 7), OPT(l0_store, 0, 2, 4), OPT(l0_scr16, 0, 2, 3), OPT(band_prows_pix, 5), OPT(band_prows_97, 6), OPT(band_prows_inv, 3), OPT(band_prows, 4),
        OPT(use_tail, 0), OPT(mega, 1, 2), OPT(deep_mid_inv, 0, 2), OPT(deep_min_planes, 1000000), OPT(deep_mid, 0), OPT(use_deep, 0), OPT(xcd_map, 1), OPT(cpl0, 4),
        OPT(force_novec, 1),
    };
    return O;
}

int main() {
    const PlanOptions def;
    std::vector<std::pair<std::string, PlanSpec>> cases, swept;
    const PlanSpec bench = frame_spec(3840, 2160, 3, 8, true, 512, 512, 6, 64, J2K_CODER_HT);
    const PlanSpec mallat_ht = frame_spec(1024, 768, 3, 8, true, 512, 512, 6, 64, J2K_CODER_HT, J2K_CLOSED_LOOP_MALLAT);
    const PlanSpec lossy = frame_spec(2048, 1080, 3, 12, false, 512, 512, 6, 64, J2K_CODER_MQ, 0, 75);
    // (six planes: too few for the deep launch, so levels 0 + 1 may be fused -- the one option the other three cannot show)
    const PlanSpec two_tiles = frame_spec(1024, 512, 3, 8, true, 512, 512, 6, 64, J2K_CODER_HT);
    swept = {{"bench4k", bench}, {"mallat_ht", mallat_ht}, {"lossy_rgb12", lossy}, {"rgb1024x512", two_tiles}};
    cases = swept;
    cases.push_back({"bench4k_c4", frame_spec(3840, 2160, 4, 8, true, 512, 512, 6, 64, J2K_CODER_HT)});
    cases.push_back({"gray2048_16", frame_spec(2048, 2048, 1, 16, true, 0, 0, 6, 64, J2K_CODER_HT)});
    cases.push_back({"rgb512_3res_cb256", frame_spec(512, 512, 3, 8, true, 0, 0, 3, 256, J2K_CODER_MQ)});
    cases.push_back({"odd_1001x747", frame_spec(1001, 747, 3, 8, true, 250, 190, 4, 64, J2K_CODER_HT)});
    cases.push_back({"tiny_1x1", frame_spec(1, 1, 1, 8, true, 0, 0, 2, 64, J2K_CODER_MQ)});
    cases.push_back({"tiny_2x3", frame_spec(2, 3, 3, 8, true, 0, 0, 2, 64, J2K_CODER_HT)});
    cases.push_back({"tiny_17x16", frame_spec(17, 16, 3, 8, true, 0, 0, 2, 64, J2K_CODER_MQ)});
    cases.push_back({"mallat_mq", frame_spec(1024, 768, 3, 8, true, 512, 512, 6, 64, J2K_CODER_MQ, J2K_CLOSED_LOOP_MALLAT)});
    cases.push_back({"mallat_c4", frame_spec(600, 400, 4, 8, true, 256, 256, 4, 64, J2K_CODER_HT, J2K_CLOSED_LOOP_MALLAT)});
    cases.push_back({"closed_ht", frame_spec(640, 480, 3, 8, true, 256, 256, 4, 64, J2K_CODER_HT, 1)});
    PlanSpec batch = bench; batch.H = 2 * 2160; batch.frame_h = 2160;
    PlanSpec shard = bench; shard.tile_first = 3; shard.tile_count = 5;
    cases.push_back({"bench4k_batch2", batch});
    cases.push_back({"bench4k_shard3_5", shard});
    cases.push_back({"unit97_f64", unit_spec(300, 200, 3, W97, Q_NONE, true)});
    cases.push_back({"unit97_tcd", unit_spec(640, 360, 4, W97, Q_TCD, false)});
    cases.push_back({"unit53", unit_spec(333, 1, 1, W53, Q_NONE, false)});
    cases.push_back({"refused_levels", unit_spec(8, 8, 33, W53, Q_NONE, false)});
    cases.push_back({"refused_size", unit_spec(65536, 32768, 1, W53, Q_NONE, false)});
    for (const auto &c : cases) run(c.first, def, c.second);
    for (const auto &c : swept)
        for (const Option &opt : options())
            for (long v : opt.values) {
                PlanOptions o;
                opt.set(o, v);
                run(c.first + "+" + opt.name + "=" + std::to_string(v), o, c.second);
            }
    if (g_bad) { fprintf(stderr, "plan_tables: %d invariant violations\n", g_bad); return 1; }
    fprintf(stderr, "plan_tables ok\n");
    return 0;
}
