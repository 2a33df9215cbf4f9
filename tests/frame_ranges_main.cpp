// frame_ranges_main.cpp -- a stand-alone driver of the frame-range builder of the rate allocation (go-jpeg2000_amd/csrc/plan_tables.h:
// frame_job_ranges; no HIP in it), built with AddressSanitizer + UBSan by tests/test_frame_rate_cases.py and run directly.  For a fixed list of
// batch geometries -- the order and the numbers of tests/frame_rate_cases.py RANGE_GEOMETRIES -- it builds the plan's tables as j2k_plan_create
// does, then prints
//   @ <name>
//   tiles <tiles in all> <tiles per frame> blocks <jobs>
//   tile <the tile of every job>
//   range <first> <count>            (one line per frame)
// and checks what the allocation kernels rely on: the ranges are in order, adjoin, and cover [0, jobs) exactly; every job of range f lies in a tile
// of frame f.  It also feeds the builder tables it must refuse (a tile out of order, a tile outside the frames).  A violation: exit status 1.
#include <cstdio>
#include <string>

#include "../go-jpeg2000_amd/csrc/plan_tables.h"

using namespace j2k;

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "INVARIANT: " __VA_ARGS__); fprintf(stderr, "\n"); g_bad++; } } while (0)

// j2k_params -> PlanSpec as j2k_plan_create makes it (a closed-loop Mallat MQ plan, lossless)
static PlanSpec batch_spec(int W, int H, int frame_rows, int C, int num_res, int cb, int tile_w, int tile_h) {
    PlanSpec S;
    S.W = W; S.H = H; S.C = C; S.frame_h = frame_rows > 0 ? frame_rows : H;
    S.tile_w = tile_w; S.tile_h = tile_h;
    S.levels = num_res - 1;
    S.wavelet = W53;
    S.precision = 8;
    S.dc_shift = 128; S.dc_shift_inv = 128;
    S.mct = C >= 3;
    S.quant = Q_NONE;
    S.quality = 100;
    S.num_res_jobs = num_res;
    S.cb_w = S.cb_h = cb;
    S.coder = J2K_CODER_MQ;
    S.closed_loop = true;
    S.mallat = true;
    return S;
}

static void run(const char *name, const PlanSpec &S) {
    printf("@ %s\n", name);
    PlanTables T;
    const char *why = "";
    const PlanLimits lim{1024, 128};
    const int r = build_plan_tables(PlanOptions(), lim, S, T, &why);
    if (r != J2K_OK) { printf("refused %d %s\n", r, why); g_bad++; return; }
    const int F = S.H / S.frame_h, tpf = T.tile_count / F;
    printf("tiles %d %d blocks %zu\ntile", T.tile_count, tpf, T.blocks.size());
    for (int32_t t : T.block_tile) printf(" %d", t);
    printf("\n");
    CHECK(T.tile_count == tpf * F, "%s: the tiles are not a whole number per frame", name);
    std::vector<RateFrame> fr;
    const bool ok = frame_job_ranges(T.block_tile, tpf, F, fr);
    CHECK(ok && (int)fr.size() == F, "%s: the builder refused the plan's own table", name);
    int next = 0;
    for (int f = 0; f < (int)fr.size(); f++) {
        printf("range %d %d\n", fr[f].first, fr[f].count);
        CHECK(fr[f].first == next && fr[f].count >= 0, "%s: frame %d does not adjoin its predecessor", name, f);
        for (int j = fr[f].first; j < fr[f].first + fr[f].count && j < (int)T.block_tile.size(); j++)
            CHECK(T.block_tile[j] / tpf == f, "%s: job %d of frame %d lies in tile %d", name, j, f, T.block_tile[j]);
        next = fr[f].first + fr[f].count;
    }
    CHECK(next == (int)T.blocks.size(), "%s: the ranges cover %d of %zu jobs", name, next, T.blocks.size());
}

int main() {
    run("untiled_batch3", batch_spec(130, 210, 70, 3, 4, 64, 0, 0));
    run("tiled_batch2_partial_rows", batch_spec(260, 88, 44, 3, 4, 64, 128, 32));
    run("single_frame", batch_spec(130, 70, 0, 3, 4, 64, 0, 0));
    run("one_sample_high", batch_spec(40, 3, 1, 1, 3, 8, 0, 0));
    // what the builder must refuse, and leave `out` empty for
    std::vector<RateFrame> fr;
    CHECK(!frame_job_ranges({0, 1, 0, 1}, 1, 2, fr) && fr.empty(), "a tile out of order was accepted");
    CHECK(!frame_job_ranges({0, 0, 2}, 1, 2, fr) && fr.empty(), "a tile outside the frames was accepted");
    CHECK(!frame_job_ranges({0}, 0, 1, fr) && fr.empty(), "zero tiles per frame were accepted");
    CHECK(frame_job_ranges({}, 2, 3, fr) && fr.size() == 3 && fr[2].first == 0 && fr[2].count == 0, "a plan without blocks: three empty frames");
    CHECK(frame_job_ranges({1, 1}, 1, 2, fr) && fr[0].count == 0 && fr[1].first == 0 && fr[1].count == 2, "a frame without blocks starts where the next one does");
    printf("@ end\n");
    return g_bad ? 1 : 0;
}
