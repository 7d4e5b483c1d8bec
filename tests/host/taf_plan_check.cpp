// taf_plan_check.cpp -- the fast path's host planner (csrc/taf_plan.h) checked on the CPU, without HIP: for every shape of the grid of
// tests/golden/workspace_bytes.json (argv[1]), three distributions of the events over the sequences, the four partition modes
// and batches_per_wave 0 / 20, what a call lays out stays inside what the size query budgets, and the plan keeps the rules
// the kernels rely on.  Built with -fsanitize=address,undefined by tests/test_taf_plan_cpu.py; exit status 0 = all held.
#include "taf_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

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

static size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// the rules of one planned and laid-out call
static void check_plan(const FastPlan &p, const SeqTab &S, const int64_t *offs, int n_seq, long long n, size_t win, size_t query)
{
    CHECK(p.bytes <= query);
    // the tables, in layout_offsets' order, with the byte lengths it takes
    const size_t n_rec = (size_t)(n > 0 ? n : 1), sub_words = (size_t)p.pairs * kFW + 1;
    CHECK(p.max_segs == 2 * (int)(n / kSplitSeg) + 1);
    const size_t off[] = {p.off_counts, p.off_slabtot, p.off_base, p.off_sub, p.off_seg0, p.off_segcnt, p.off_errs, p.off_tlut,
                          p.off_records, p.off_records2, p.off_sub_end, p.off_segdesc, p.off_wst, p.off_wst_flag};
    const size_t len[] = {(size_t)p.chunks * p.TB * 4, (size_t)p.slabs * p.TB * 4, (size_t)(p.pairs_b + 1) * 4, sub_words * 4,
                          (size_t)(p.pairs_b + 1) * 4, (size_t)p.max_segs * kFW * 4, (size_t)p.chunks * 4, (win + 1) * 4,
                          n_rec * 4, n_rec * 4, sub_words * 4, (size_t)p.max_segs * 4,
                          (size_t)p.pairs * kFW * (FRLW_MAX_WINDOWS + 1) * 4, (size_t)p.pairs * 4};
    const int n_tab = (int)(sizeof(off) / sizeof(off[0]));
    CHECK(off[0] == kHeaderBytes);
    for (int i = 0; i < n_tab; ++i) {
        CHECK(off[i] % 256 == 0 && off[i] >= kHeaderBytes);
        const size_t next = i + 1 < n_tab ? off[i + 1] : p.bytes; // ascending, no overlap, no more than the alignment in between
        CHECK(off[i] + len[i] <= next && next - (off[i] + len[i]) < 256);
    }
    CHECK(p.bytes % 256 == 0);
    // chunk size
    const long long cap = (long long)kFT * (p.big ? kBigBpw : kMaxBpw);
    const long long lds_cap = ((79ll * 1024 - 16 - (long long)kFW * p.TB * 4 - (p.TB + 2) * 4) / 6) / 16 * 16; // fast_plan's direct-mode cap
    CHECK(p.chunk % 16 == 0 && p.chunk <= cap);
    CHECK(p.chunk >= 1024 || (p.direct && p.chunk >= lds_cap));
    CHECK(p.bpw == (int)ceil_div(ceil_div((size_t)p.chunk, 16), 64));
    // the per-sequence tables
    int max_cs = 1;
    CHECK(S.n_seq == n_seq && S.chunk0[0] == 0 && S.slab0[0] == 0);
    for (int s = 0; s < n_seq; ++s) {
        const long long n_s = offs[s + 1] - offs[s];
        int cs = (int)ceil_div((size_t)n_s, (size_t)p.chunk);
        if (cs < 1) cs = 1;
        if (cs > max_cs) max_cs = cs;
        CHECK(S.chunk0[s + 1] - S.chunk0[s] == cs);
        CHECK(S.slab0[s + 1] - S.slab0[s] == (int)ceil_div((size_t)cs, kFastSlab));
        CHECK(S.ev0[s] == offs[s]);
    }
    CHECK(S.ev0[n_seq] == offs[n_seq]);
    CHECK(p.max_seq_chunks == max_cs);
    CHECK(p.chunks == S.chunk0[n_seq] && p.slabs == S.slab0[n_seq]);
    // modes
    if (p.direct) CHECK(kFW * p.T <= kMaxFastTiles && (long long)kFW * p.T * n_seq <= kMaxBinPairs && p.TB == kFW * p.T);
    if (p.big) CHECK(!p.direct);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: taf_plan_check tests/golden/workspace_bytes.json\n"); return 2; }
    std::string text;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, k);
        fclose(f);
    }
    const std::vector<long long> events = json_ints(text, "events"), seqs = json_ints(text, "sequences"), frames = json_ints(text, "frames_h_w"),
                                 windows = json_ints(text, "windows_us"), golden = json_ints(text, "bytes");
    if (events.empty() || seqs.empty() || frames.empty() || frames.size() % 2 || windows.empty() ||
        golden.size() != events.size() * seqs.size() * (frames.size() / 2) * windows.size()) {
        fprintf(stderr, "%s: not the grid this program expects\n", argv[1]);
        return 2;
    }
    long long planned = 0, refused = 0, calls = 0;
    size_t gi = 0;
    for (long long n : events)
        for (long long n_seq_ll : seqs)
            for (size_t fi = 0; fi < frames.size(); fi += 2)
                for (long long win : windows) {
                    const int n_seq = (int)n_seq_ll, H = (int)frames[fi], W = (int)frames[fi + 1];
                    char ctx[160];
                    snprintf(ctx, sizeof(ctx), "n=%lld n_seq=%d H=%d W=%d window=%lld", n, n_seq, H, W, win);
                    g_ctx = ctx;
                    const size_t query = batch_workspace_bytes(n, n_seq, H, W, win);
                    CHECK(query == (size_t)golden[gi++]);
                    FastPlan p;
                    SeqTab S;
                    bool cm = false;
                    int64_t offs[kMaxSeq + 1], t0[kMaxSeq] = {};
                    if (query == 0) { // a refused shape: no mode plans it
                        for (int s = 0; s <= n_seq; ++s) offs[s] = s ? n : 0;
                        CHECK(plan_select(CM_AUTO, 0, -1, false, n_seq, H, W, offs, t0, win, p, S, cm) != FRLW_OK);
                        ++refused;
                        continue;
                    }
                    ++planned;
                    for (int dist = 0; dist < 3; ++dist) {
                        // 0: everything in the first sequence; 1: an even split; 2: full and empty sequences in turn (the first one full)
                        const int n_full = (n_seq + 1) / 2;
                        for (int s = 0; s <= n_seq; ++s)
                            offs[s] = dist == 0 ? (s ? n : 0) : dist == 1 ? n * s / n_seq : n * ((s + 1) / 2) / n_full;
                        for (int mode = 0; mode < 16; ++mode) {
                            const int direct = mode & 1, knob_cm = (mode >> 1) & 1 ? CM_ON : CM_OFF, bpw = (mode >> 2) & 1 ? 20 : 0;
                            const bool ev = (mode >> 3) & 1;
                            snprintf(ctx, sizeof(ctx), "n=%lld n_seq=%d H=%d W=%d window=%lld dist=%d direct=%d cm=%d bpw=%d ev=%d", n, n_seq,
                                     H, W, win, dist, direct, knob_cm, bpw, (int)ev);
                            g_ctx = ctx;
                            const int rc = plan_select(knob_cm, bpw, direct, ev, n_seq, H, W, offs, t0, win, p, S, cm);
                            CHECK(rc == FRLW_OK);
                            if (rc != FRLW_OK) continue;
                            ++calls;
                            check_plan(p, S, offs, n_seq, n, (size_t)win, query);
                            if (!direct) CHECK(!p.direct);
                            if (knob_cm == CM_OFF) CHECK(!cm && !p.big);
                            // a chunk-major call's consumer holds the longest sequence's column in LDS
                            // (the sizes as numbers, from the consumers' LDS arrays: kf_ev_sub / kf_ev_fadd / kf_sae_sub 511 + 1 words,
                            // kf_taf_walk<., true> 2047 + 1, the split kernels 4096 + 1 -- not through the constants cm_fits reads)
                            const int col = p.direct ? (ev ? 511 : 2047) : 4096;
                            if (cm) CHECK(p.max_seq_chunks <= col && p.chunk <= 65535);
                            if (p.max_seq_chunks > col) CHECK(!cm_fits(p, ev));
                            if (knob_cm == CM_ON && !cm) { // the chunk-major plan of the same call was turned down: because it did not fit
                                FastPlan pc;
                                SeqTab Sc;
                                CHECK(fast_plan(n, n_seq, H, W, pc, direct ? DIRECT_FORCE : DIRECT_OFF, bpw, true) &&
                                      fast_layout(offs, t0, n_seq, pc, Sc, (uint32_t)win) && !cm_fits(pc, ev));
                                const int colc = pc.direct ? (ev ? 511 : 2047) : 4096;
                                CHECK(pc.max_seq_chunks > colc || pc.chunk > 65535);
                            }
                        }
                    }
                }
    // the SAE / Event Count Image two-launch form: both ends of its eligibility at 304 x 240
    {
        const long long ns[4] = {16383, 16384, (1ll << 20) - 2, (1ll << 20) - 1};
        const bool want[4] = {false, true, true, false};
        for (int i = 0; i < 4; ++i) {
            char ctx[64];
            snprintf(ctx, sizeof(ctx), "sae_fast_plan n=%lld", ns[i]);
            g_ctx = ctx;
            FastPlan p;
            SeqTab S;
            const bool ok = sae_fast_plan(ns[i], 240, 304, 0, p, S);
            CHECK(ok == want[i]);
            if (ok) {
                CHECK(p.direct && !p.big && p.max_seq_chunks <= 511 && p.chunk <= 65535);
                CHECK(scatter_cm_lds_bytes(p.TB, p.chunk) <= 160 * 1024);
                const int64_t offs[2] = {0, (int64_t)ns[i]};
                check_plan(p, S, offs, 1, ns[i], 1, (size_t)-1); // (this form's size query IS the plan's bytes: nothing to compare)
            }
        }
    }
    printf("taf_plan_check: %lld planned shapes, %lld refused, %lld calls, %lld checks, %lld failed\n", planned, refused, calls, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
