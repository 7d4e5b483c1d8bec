// enc_plan_check.cpp -- the general path's host planner (csrc/enc_plan.h) checked on the CPU, without HIP: for every event count and
// frame of the grid of tests/golden/encoder_workspace_bytes.json (argv[1]) plus frames that cross the tile-widening and refusal
// branches, each crossed with every knob of the general path at its default, at both ends of its range and one step outside, the
// plan keeps the rules the kernels rely on, the scatter's LDS fits the CU and the tile grid is the one the kernels decode.
// Built with -fsanitize=address,undefined by tests/test_enc_plan_cpu.py; exit status 0 = all held.
#include "enc_plan.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

using namespace frlw;

static long long g_checks = 0, g_failed = 0;
static std::string g_ctx;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        ++g_checks;                                                                           \
        if (!(cond) && ++g_failed <= 20) fprintf(stderr, "FAILED %s  [%s]\n", #cond, g_ctx.c_str()); \
    } while (0)

// the integers of the (possibly nested) array behind "key": in the JSON text
static std::vector<long long> json_ints(const std::string &text, const char *key)
{
    std::vector<long long> out;
    size_t at = text.find(std::string("\"") + key + "\":");
    if (at == std::string::npos) return out;
    at = text.find('[', at);
    for (int depth = 0; at < text.size(); ++at) {
        const char c = text[at];
        if (c == '[') ++depth;
        else if (c == ']') { if (--depth == 0) break; }
        else if (c >= '0' && c <= '9') {
            char *end = nullptr;
            out.push_back(strtoll(text.c_str() + at, &end, 10));
            at = (size_t)(end - text.c_str()) - 1;
        }
    }
    return out;
}

struct Knobs { // -1 = the library's choice
    const char *name;
    int twl, bpw, hot, staged, quarter, no_lut;
};

static frlw_tuning_t tuning_of(const Knobs &k)
{
    frlw_tuning_t t;
    memset(&t, 0xff, sizeof(t)); // every field -1
    t.struct_size = (int32_t)sizeof(t);
    t.tile_width_log2 = k.twl; t.batches_per_wave = k.bpw; t.hot_tile_records = k.hot;
    t.staged_scatter = k.staged; t.quarter_below = k.quarter; t.no_value_table = k.no_lut;
    return t;
}

// the rules of one planned call
static void check_plan(const Plan &p, long long n, int H, int W, const Knobs &k)
{
    // tiles: (1 << twl) x kTileH pixels, covering the frame; the narrowest width from the requested one on that fits, else 8
    const int want_twl = k.twl >= 0 ? k.twl : (W > 512 ? 8 : 6);
    CHECK(p.twl >= 6 && p.twl <= 8 && p.twl >= want_twl);
    CHECK((long long)p.tiles_x << p.twl >= W && (long long)(p.tiles_x - 1) << p.twl < W);
    CHECK((long long)p.tiles_y * 8 >= H && (long long)(p.tiles_y - 1) * 8 < H);
    CHECK(p.n_tiles == p.tiles_x * p.tiles_y && p.n_tiles >= 1 && p.n_tiles <= 2048); // k_tilescan's tot[kMaxTiles]
    for (int t = want_twl; t < p.twl; ++t) // every narrower width was too many tiles
        CHECK((long long)((W + (1 << t) - 1) >> t) * ((H + 7) / 8) > 2048);
    // chunks: one partition workgroup of 1024 threads takes bpw batches of 64 events per wavefront
    CHECK(p.bpw >= 1 && p.bpw <= 8); // q[kMaxBpw], where[kMaxBpw] of k_hist / k_scatter
    if (k.bpw >= 0) CHECK(p.bpw == k.bpw);
    CHECK(p.chunk == 1024ll * p.bpw);
    CHECK(p.units >= 1 && (long long)p.units * p.chunk >= n && (p.units == 1 || (long long)(p.units - 1) * p.chunk < n));
    CHECK(p.slabs >= 1 && (long long)p.slabs * 32 >= p.units && (long long)(p.slabs - 1) * 32 < p.units); // k_scatter reads slab wg / 32
    // the six regions behind the header, in order, 256-aligned, disjoint, each as long as what the kernels index:
    //   counts[wg * n_tiles + b], wg < units (k_hist)         slabtot[slab * n_tiles + b], slab < slabs (k_slabscan)
    //   base[0 .. n_tiles] (k_tilescan)                        errs[wg] (k_hist)
    //   tlut_w[r], r <= win <= 65536 (k_hist, partition_events) records[pos], pos < n (k_scatter)
    const size_t off[] = {p.off_counts, p.off_slabtot, p.off_base, p.off_errs, p.off_tlut, p.off_records};
    const size_t len[] = {(size_t)p.units * p.n_tiles * 4, (size_t)p.slabs * p.n_tiles * 4, (size_t)(p.n_tiles + 1) * 4,
                          (size_t)p.units * 4, (size_t)(65536 + 1) * 4, (size_t)(n > 0 ? n : 1) * 8};
    CHECK(off[0] == 1024 && kHeaderBytes == 1024);
    for (int i = 0; i < 6; ++i) {
        const size_t next = i + 1 < 6 ? off[i + 1] : p.bytes;
        CHECK(off[i] % 256 == 0 && off[i] >= kHeaderBytes);
        CHECK(off[i] + len[i] <= next && next - (off[i] + len[i]) < 256);
    }
    CHECK(p.bytes % 256 == 0);
    // knobs
    if (k.hot >= 0) CHECK(p.hot_thr == (unsigned)k.hot);
    else {
        const long long slice2 = 2ll * 16 * (4 << p.twl), mean4 = 4 * (n / p.n_tiles), thr = slice2 > mean4 ? slice2 : mean4;
        CHECK(p.hot_thr == (unsigned)(thr > INT_MAX ? INT_MAX : thr));
    }
    CHECK(p.staged == k.staged && p.quarter_below == (k.quarter >= 0 ? k.quarter : 1024) && p.no_lut == (k.no_lut >= 0 ? k.no_lut : 0));
    // the scatter workgroup's LDS: gs u32 per tile | wcnt u16 per (wave, tile rounded to even) | tag u8 per (wave, tile); the staged
    // form adds, 16-aligned, loff u32 per tile + 2 (rounded to even) | 4096 staged records of 8 bytes | their 4096 u16 tiles
    const ScatterLds l = scatter_lds(p, n);
    const size_t nt = (size_t)p.n_tiles, nt2 = (nt + 1) & ~(size_t)1;
    const size_t direct_end = nt * 4 + 16 * nt2 * 2 + 16 * nt;
    CHECK(l.hist == nt * 4 && l.hist <= 64 * 1024);
    CHECK(l.direct >= direct_end && l.direct <= 160 * 1024); // the MI355X's LDS per CU
    CHECK(stage_off(p.n_tiles) >= direct_end && stage_off(p.n_tiles) % 16 == 0);
    CHECK(l.staged_bytes >= stage_off(p.n_tiles) + ((nt + 2 + 1) & ~(size_t)1) * 4 + 4096 * 8 + 4096 * 2);
    const bool asked = p.staged >= 0 ? p.staged != 0 : (p.bpw >= 4 && n >= 3000000);
    CHECK(l.staged == (asked && l.staged_bytes <= 150 * 1024));
    // the tile grid of the Event Volume / TAF kernels
    const TileGrid g = tile_grid(p);
    const bool quarters = (long long)p.n_tiles * ((4 << p.twl) / 64) <= p.quarter_below;
    CHECK(g.all_quarters == quarters);
    CHECK(g.blocks == (quarters ? 4 * p.n_tiles : p.n_tiles + 4 * 32));
    CHECK(g.n_tiles_arg == (quarters ? -p.n_tiles : p.n_tiles));
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: enc_plan_check tests/golden/encoder_workspace_bytes.json\n"); return 2; }
    std::string text;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, k);
        fclose(f);
    }
    const std::vector<long long> events = json_ints(text, "events"), frames = json_ints(text, "frames_h_w"), golden = json_ints(text, "bytes");
    if (events.size() != 8 || frames.size() != 24 || golden.size() != events.size() * (frames.size() / 2)) {
        fprintf(stderr, "%s: not the grid this program expects\n", argv[1]);
        return 2;
    }
    const Knobs knobs[] = {
        {"default", -1, -1, -1, -1, -1, -1},
        {"twl=5", 5, -1, -1, -1, -1, -1}, {"twl=6", 6, -1, -1, -1, -1, -1}, {"twl=7", 7, -1, -1, -1, -1, -1},
        {"twl=8", 8, -1, -1, -1, -1, -1}, {"twl=9", 9, -1, -1, -1, -1, -1},
        {"bpw=0", -1, 0, -1, -1, -1, -1}, {"bpw=1", -1, 1, -1, -1, -1, -1}, {"bpw=8", -1, 8, -1, -1, -1, -1}, {"bpw=9", -1, 9, -1, -1, -1, -1},
        {"hot=0", -1, -1, 0, -1, -1, -1}, {"hot=max", -1, -1, INT_MAX, -1, -1, -1},
        {"staged=0", -1, -1, -1, 0, -1, -1}, {"staged=1", -1, -1, -1, 1, -1, -1}, {"staged=2", -1, -1, -1, 2, -1, -1},
        {"quarter=0", -1, -1, -1, -1, 0, -1}, {"quarter=max", -1, -1, -1, -1, INT_MAX, -1},
        {"no_lut=0", -1, -1, -1, -1, -1, 0}, {"no_lut=1", -1, -1, -1, -1, -1, 1}, {"no_lut=2", -1, -1, -1, -1, -1, 2},
    };
    // the frames of the fixture (among them: too many tiles at width 6 but not at 7, too many at 7 but not at 8, and two that are
    // refused at width 8) plus shapes that are not positive
    std::vector<long long> fr(frames);
    const long long extra[] = {0, 5, 5, -1};
    fr.insert(fr.end(), extra, extra + 4);
    std::vector<long long> ns(events);
    ns.push_back(-1);
    long long planned = 0, refused = 0, widened7 = 0, widened8 = 0, staged = 0, quarters = 0;
    for (size_t ni = 0; ni < ns.size(); ++ni)
        for (size_t fi = 0; fi < fr.size(); fi += 2)
            for (const Knobs &k : knobs) {
                const long long n = ns[ni];
                const int H = (int)fr[fi], W = (int)fr[fi + 1];
                char ctx[160];
                snprintf(ctx, sizeof(ctx), "n=%lld H=%d W=%d %s", n, H, W, k.name);
                g_ctx = ctx;
                const frlw_tuning_t tu = tuning_of(k);
                Plan p;
                const bool ok = make_plan(n, H, W, strcmp(k.name, "default") ? &tu : nullptr, p);
                // refused exactly for: a shape that is not positive, n < 0, a knob outside its range, more than 2048 tiles at width 8
                const bool shape_bad = H <= 0 || W <= 0 || n < 0;
                const bool knob_bad = (k.twl >= 0 && (k.twl < 6 || k.twl > 8)) || (k.bpw >= 0 && (k.bpw < 1 || k.bpw > 8));
                const bool too_many = !shape_bad && (long long)((W + 255) / 256) * ((H + 7) / 8) > 2048;
                CHECK(ok == !(shape_bad || knob_bad || too_many));
                if (ni < events.size() && fi < frames.size() && !strcmp(k.name, "default")) {
                    // the size query is max(this plan, the two-launch form's plan): never less than the plan, 0 exactly when refused
                    const long long q = golden[ni * (frames.size() / 2) + fi / 2];
                    CHECK((q == 0) == !ok);
                    if (ok) CHECK((long long)p.bytes <= q);
                }
                if (!ok) { ++refused; continue; }
                ++planned;
                check_plan(p, n, H, W, k);
                const int want_twl = k.twl >= 0 ? k.twl : (W > 512 ? 8 : 6);
                widened7 += p.twl == 7 && want_twl < 7;
                widened8 += p.twl == 8 && want_twl < 8;
                staged += scatter_lds(p, n).staged;
                quarters += tile_grid(p).all_quarters;
            }
    // a knob behind the caller's struct_size takes the default; a struct_size outside [8, 4096] is invalid
    {
        g_ctx = "struct_size";
        frlw_tuning_t tu = tuning_of(knobs[4]); // twl = 8
        tu.batches_per_wave = 9;                // would be refused if it were read
        tu.struct_size = 8;                     // struct_size + tile_width_log2
        Plan p;
        CHECK(tuning_valid(&tu) && make_plan(1000, 240, 304, &tu, p) && p.twl == 8 && p.bpw == 1);
        tu.struct_size = 4;
        CHECK(!tuning_valid(&tu) && make_plan(1000, 240, 304, &tu, p) && p.twl == 6);
        tu.struct_size = 4097;
        CHECK(!tuning_valid(&tu));
        CHECK(tuning_valid(nullptr));
    }
    CHECK(widened7 > 0 && widened8 > 0 && staged > 0 && quarters > 0 && quarters < planned);
    printf("enc_plan_check: %lld planned, %lld refused, %lld widened to 7, %lld widened to 8, %lld staged, %lld all-quarters, %lld checks, %lld failed\n",
           planned, refused, widened7, widened8, staged, quarters, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
