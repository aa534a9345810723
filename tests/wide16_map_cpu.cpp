// Stand-alone host program of tests/test_wide16_map_cpu.py: the tile map of the skewed 256 x 256 ConvLSTM form (csrc/conv_route.cpp
// wide16_tile_map / conv_plan_wide16_map).  Compiled together with csrc/conv_route.cpp alone, no HIP call.  It walks every map the way
// the kernel does (range = block % 8, place = block / 8, M tile = place / N tiles; full tiles first, 192-pixel ones behind them) and
// checks the properties itself; the headline launches' rows are printed as JSON lines for the test to read.  Exit status 1 and a line
// per violation on stderr when a property fails.
#include "conv_route.h"
#include <cstdio>
#include <map>
#include <string>
#include <vector>

using namespace evr;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_bad; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
static ConvKnobs knobs(std::map<std::string, std::string> env) { g_env = env; return conv_knobs_from(lookup); }

// the kernel's decode of (range, M tile) -> first pixel and height; 0 rows: the block leaves at once
static void decode(const Wide16Map& m, int x, int mt, int64_t* m0, int* rows) {
    if (mt >= m.count[x]) { *rows = 0; *m0 = -1; return; }
    const int nf = m.full[x];
    *rows = mt < nf ? 256 : 192;
    *m0 = m.pix0[x] + (mt < nf ? (int64_t)mt * 256 : (int64_t)nf * 256 + (int64_t)(mt - nf) * 192);
}

// every pixel in exactly one tile, ranges and tiles end to end, short tiles last, no empty tile, only the last tile past M
static void check_cover(const char* what, const Wide16Map& m, int64_t M, bool count_pixels) {
    std::vector<unsigned char> seen(count_pixels ? (size_t)M : 0, 0);
    int64_t next = 0;
    bool range_ended_early = false;
    for (int x = 0; x < 8; ++x) {
        CHECK(m.count[x] >= 0 && m.count[x] <= m.slots && m.full[x] >= 0 && m.full[x] <= m.count[x], "%s range %d: count %d full %d slots %d", what, x, m.count[x], m.full[x], m.slots);
        CHECK(!range_ended_early || m.count[x] == 0, "%s range %d: tiles behind a range that was not full", what, x);
        if (m.count[x] < m.slots) range_ended_early = true;
        bool short_seen = false;
        for (int mt = 0; mt < m.slots; ++mt) {
            int64_t m0; int rows;
            decode(m, x, mt, &m0, &rows);
            if (!rows) continue;
            CHECK(m0 == next, "%s range %d tile %d starts at %lld, the one before ended at %lld", what, x, mt, (long long)m0, (long long)next);
            CHECK(m0 < M, "%s range %d tile %d holds no pixel", what, x, mt);
            CHECK(!(short_seen && rows == 256), "%s range %d tile %d: a full tile behind a short one", what, x, mt);
            if (rows == 192) short_seen = true;
            for (int64_t p = m0; count_pixels && p < m0 + rows && p < M; ++p) if (p >= 0) ++seen[(size_t)p];
            CHECK(m0 + rows <= M || m0 + rows - M < rows, "%s tile past M", what);
            next = m0 + rows;
            if (next > M) { CHECK(next - M < rows, "%s: more than the last tile is past M", what); next = M; range_ended_early = true; }
        }
    }
    CHECK(next == M, "%s: tiles end at %lld of %lld pixels", what, (long long)next, (long long)M);
    for (size_t p = 0; p < seen.size(); ++p) if (seen[p] != 1) { CHECK(seen[p] == 1, "%s: pixel %zu in %d tiles", what, p, (int)seen[p]); break; }
}

static int shorts_of(const Wide16Map& m) { int n = 0; for (int x = 0; x < 8; ++x) n += m.count[x] - m.full[x]; return n; }
static int tiles_of(const Wide16Map& m) { int n = 0; for (int x = 0; x < 8; ++x) n += m.count[x]; return n; }

// a ConvLSTM gate convolution ready for the h3 kernels (tests/conv_route_cpu.cpp's conv_same)
static ConvArgs lstm(int n, int h, int w, int c0, int c1, int hidden) {
    ConvArgs a = {};
    a.n = n; a.hin = a.hm = a.hout = h; a.win = a.wm = a.wout = w;
    a.c0 = c0; a.c1 = c1; a.in_mode = IN_CAT;
    a.stride = 1; a.os = 1; a.cout = 4 * hidden; a.n_valid = a.cout; a.cout_total = a.cout; a.epi = EPI_LSTM; a.hidden = hidden;
    a.tp.ntaps = 9; a.tp.ngroups = 1; a.tp.grp_cols = a.cout;
    for (int t = 0; t < 9; ++t) a.tp.set_tap(t, t / 3 - 1, t % 3 - 1, 1);
    a.x3 = 3; a.in_packed = 1; a.acc_scale = 1.f;
    return a;
}

int main() {
    // ---- the three headline launches: 64 sequences of 346 x 260 (padded 352 x 264), 256 CUs
    const struct { const char* name; int h, w, c, hidden; } L[3] = {{"enc0.rec", 132, 176, 64, 64}, {"enc1.rec", 66, 88, 128, 128}, {"enc2.rec", 33, 44, 256, 256}};
    for (const auto& l : L) {
        ConvArgs a = lstm(64, l.h, l.w, l.c, l.c, l.hidden);
        const int64_t M = (int64_t)a.n * a.hm * a.wm;
        const int nt = a.cout / 256;
        const ConvKnobs k = knobs({});
        const Wide16Plan p = wide16_tile_map(M, nt, 256, k.wide16_short, k.wide16_short_last);
        CHECK(p.map.slots > 0, "%s: the rule leaves the headline launch alone", l.name);
        check_cover(l.name, p.map, M, true);
        for (int x = 0; x < 8; ++x) CHECK(p.map.count[x] == p.map.slots, "%s: range %d has %d tiles, others %d", l.name, x, p.map.count[x], p.map.slots);
        CHECK(p.makespan < p.makespan_uniform, "%s: makespan %f against %f", l.name, p.makespan, p.makespan_uniform);
        // through the plan and the route: the grid is the map's, whole rounds of 256 blocks
        conv_plan_wide16_map(a, 32, 4, 4, 256, k);
        const ConvRoute r = conv_route(a, 32, 4, 4, k);
        CHECK(r.family == CONV_WIDE16 && r.short16 && r.grid == 8u * p.map.slots * nt && r.grid % 256 == 0, "%s: route grid %u short16 %d", l.name, r.grid, (int)r.short16);
        CHECK(memcmp(&a.w16map, &p.map, sizeof(p.map)) == 0, "%s: the plan's map is not the rule's", l.name);
        // EVR_WIDE16_SHORT=0: the uniform map, the parent's grid
        ConvArgs a0 = lstm(64, l.h, l.w, l.c, l.c, l.hidden);
        const ConvKnobs k0 = knobs({{"EVR_WIDE16_SHORT", "0"}});
        conv_plan_wide16_map(a0, 32, 4, 4, 256, k0);
        const ConvRoute r0 = conv_route(a0, 32, 4, 4, k0);
        const Wide16Plan p0 = wide16_tile_map(M, nt, 256, k0.wide16_short, 0);
        CHECK(a0.w16map.slots == 0 && p0.map.slots == 0 && !r0.short16 && r0.grid == (unsigned)(((M + 255) / 256) * nt) && p0.mtiles == (int)((M + 255) / 256) && p0.nshort == 0,
              "%s: EVR_WIDE16_SHORT=0 grid %u", l.name, r0.grid);
        // an explicit EVR_WIDE_MIN keeps the rule out (the forced modes are not the rule)
        ConvArgs a1 = lstm(64, l.h, l.w, l.c, l.c, l.hidden);
        const ConvKnobs k1 = knobs({{"EVR_WIDE", "3"}, {"EVR_WIDE_MIN", "1"}});
        conv_plan_wide16_map(a1, 32, 4, 4, 256, k1);
        CHECK(a1.w16map.slots == 0, "%s: the rule under an explicit EVR_WIDE_MIN", l.name);
        printf("{\"id\": \"%s\", \"M\": %lld, \"nt\": %d, \"full\": %d, \"short\": %d, \"grid\": %u, \"grid_uniform\": %u, \"makespan\": %.4f, \"makespan_uniform\": %.1f}\n",
               l.name, (long long)M, nt, p.mtiles - p.nshort, p.nshort, r.grid, r0.grid, p.makespan, p.makespan_uniform);
    }
    // ---- below the form's own threshold and on the twin form nothing changes (16 sequences: enc2.rec is 363 tiles; 32: enc0.rec twin)
    {
        const ConvKnobs k = knobs({});
        ConvArgs a = lstm(16, 33, 44, 256, 256, 256);
        conv_plan_wide16_map(a, 32, 4, 4, 256, k);
        CHECK(a.w16map.slots == 0 && !conv_route(a, 32, 4, 4, k).short16, "enc2.rec at 16 sequences got a map");
        ConvArgs b = lstm(32, 132, 176, 64, 64, 64);
        conv_plan_wide16_map(b, 32, 4, 4, 256, k);
        CHECK(b.w16map.slots == 0 && conv_route(b, 32, 4, 4, k).wn == 1, "enc0.rec at 32 sequences (twin form) got a map");
        // EVR_WIDE16_TAIL=0 / EVR_WIDE16_ALT=0: the kernels without the short path keep the uniform map
        for (const char* sw : {"EVR_WIDE16_TAIL", "EVR_WIDE16_ALT"}) {
            ConvArgs c = lstm(64, 66, 88, 128, 128, 128);
            const ConvKnobs ks = knobs({{sw, "0"}, {"EVR_WIDE16_SHORT", "all"}});
            conv_plan_wide16_map(c, 32, 4, 4, 256, ks);
            CHECK(c.w16map.slots == 0 && !conv_route(c, 32, 4, 4, ks).short16, "%s=0 got a map", sw);
        }
    }
    // ---- the rule over small and degenerate M, nt and C; whenever it gives a map: cover, equal counts, a / b by the formula
    int rule_maps = 0;
    for (int cus : {8, 16, 32, 64, 104, 128, 256, 304, 0, 7, 12})
        for (int nt : {1, 2, 4, 8})
            for (int64_t M : {1LL, 63LL, 64LL, 191LL, 192LL, 193LL, 255LL, 256LL, 257LL, 1000LL, 2047LL, 2048LL, 4097LL, 16385LL, 65535LL, 92928LL, 100001LL, 371712LL}) {
                const Wide16Plan p = wide16_tile_map(M, nt, cus, WIDE16_SHORT_RULE, 0);
                char what[96];
                snprintf(what, sizeof(what), "rule M=%lld nt=%d cus=%d", (long long)M, nt, cus);
                if (p.map.slots == 0) { CHECK(p.mtiles == (int)((M + 255) / 256) && p.nshort == 0, "%s: uniform totals", what); continue; }
                ++rule_maps;
                CHECK(cus > 0 && cus % (8 * nt) == 0, "%s: a map for a CU count the ranges do not divide", what);
                check_cover(what, p.map, M, M <= 100001);
                const int64_t per_round = cus / nt, R = (M + 256 * per_round - 1) / (256 * per_round), Mt = R * per_round;
                const int64_t b = std::min<int64_t>(Mt, (256 * Mt - M) / 64);
                CHECK(tiles_of(p.map) == Mt && shorts_of(p.map) == b && p.mtiles == Mt && p.nshort == b, "%s: %d tiles %d short, formula %lld / %lld", what, tiles_of(p.map), shorts_of(p.map), (long long)Mt, (long long)b);
                for (int x = 0; x < 8; ++x) CHECK(p.map.count[x] == p.map.slots, "%s: unequal ranges", what);
                CHECK(p.makespan <= p.makespan_uniform - WIDE16_SHORT_MARGIN, "%s: taken without the margin", what);
            }
    CHECK(rule_maps > 20, "the sweep met only %d maps of the rule", rule_maps);
    // ---- the forced modes (tests, measuring a short tile): any M
    for (int64_t M : {1LL, 24LL, 45LL, 96LL, 180LL, 191LL, 192LL, 193LL, 256LL, 384LL, 720LL, 1024LL, 1535LL, 1536LL, 1537LL, 2880LL, 7000LL, 92928LL}) {
        char what[96];
        const Wide16Plan pa = wide16_tile_map(M, 2, 256, WIDE16_SHORT_ALL, 0);
        snprintf(what, sizeof(what), "all M=%lld", (long long)M);
        check_cover(what, pa.map, M, true);
        CHECK(pa.map.slots > 0 && shorts_of(pa.map) == tiles_of(pa.map) && tiles_of(pa.map) == (M + 191) / 192, "%s: %d tiles, %d short", what, tiles_of(pa.map), shorts_of(pa.map));
        for (int k : {1, 2, 5, 1000}) {
            const Wide16Plan pl = wide16_tile_map(M, 2, 256, WIDE16_SHORT_LAST, k);
            snprintf(what, sizeof(what), "last=%d M=%lld", k, (long long)M);
            check_cover(what, pl.map, M, true);
            CHECK(pl.map.slots > 0, "%s: no map", what);
            for (int x = 0; x < 8; ++x)
                CHECK(pl.map.count[x] < pl.map.slots || pl.map.count[x] - pl.map.full[x] == std::min(k, pl.map.slots), "%s: range %d is full with %d short tiles", what, x, pl.map.count[x] - pl.map.full[x]);
        }
    }
    // ---- the switch's spellings
    CHECK(knobs({}).wide16_short == WIDE16_SHORT_RULE && knobs({{"EVR_WIDE16_SHORT", "1"}}).wide16_short == WIDE16_SHORT_RULE, "default / 1");
    CHECK(knobs({{"EVR_WIDE16_SHORT", "0"}}).wide16_short == WIDE16_SHORT_OFF && knobs({{"EVR_WIDE16_SHORT", "all"}}).wide16_short == WIDE16_SHORT_ALL, "0 / all");
    { const ConvKnobs k = knobs({{"EVR_WIDE16_SHORT", "last=3"}}); CHECK(k.wide16_short == WIDE16_SHORT_LAST && k.wide16_short_last == 3, "last=3"); }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    return 0;
}
