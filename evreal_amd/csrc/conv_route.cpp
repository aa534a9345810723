// conv_route(): from a convolution's launch plan to the kernel, template arguments, grid and split-K count it runs with.
// The order of the tests is the order of preference: c16, programmed band, 5x5 band, narrow 3x3 band, 3x3 band, implicit GEMM.
// Which object carries a kernel follows from a.x3, which each object of conv.hip requires to be its own: 3 = h3 (c16, wide16),
// 4 = m6, 0 / 2 = mx (the exact-fp32 implicit GEMM with its REGSTAGE ConvLSTM and KC = 16 cases).
#include "conv_route.h"
#include <algorithm>
#include <vector>

namespace evr {

ConvKnobs conv_knobs_from(const char* (*get)(const char*)) {
    ConvKnobs k;
    // (the parse idioms are knobs.h's)
    const auto num = [&](const char* name, int dflt) { return knob_num(get, name, dflt); };
    const auto second = [&](const char* name, int dflt) { return knob_second(get, name, dflt); };
    const auto set = [&](const char* name) { return knob_set(get, name); };
    const auto on = [&](const char* name) { return knob_on(get, name); };
    k.no_band = set("EVR_NO_BAND");
    k.band_min = num("EVR_BAND_MIN", 1);
    k.band5 = !(k.no_band || !on("EVR_BAND5"));
    k.band5_min = set("EVR_BAND_MIN") ? k.band_min : num("EVR_BAND5_MIN", 1);
    k.band_prog_all = on("EVR_BAND_PROG_ALL");
    k.prog_wide = num("EVR_PROG_WIDE", 1);
    k.prog_wide_min = num("EVR_PROG_WIDE_MIN", 600);
    k.ksplit = num("EVR_KSPLIT", 4);
    k.ksplit_small = num("EVR_KSPLIT_SMALL", set("EVR_KSPLIT") ? 0 : 8);
    k.ksplit_epi4 = num("EVR_KSPLIT_EPI4", 1);
    k.wide = num("EVR_WIDE", 1);
    k.wide_min = num("EVR_WIDE_MIN", 600);
    k.wide_min_set = set("EVR_WIDE_MIN");
    k.wide_min_twin = k.wide_min_set ? k.wide_min : 350;
    k.wide_min_dec32 = k.wide_min_set ? k.wide_min : 350;
    k.wide_min_plain = num("EVR_WIDE_MIN_PLAIN", k.wide_min > 1024 ? k.wide_min : (k.wide_min_set ? k.wide_min : 1024));
    k.wide_dec = num("EVR_WIDE_DEC", 1);
    k.mfma16 = num("EVR_MFMA16", 1);
    k.wide16_alt = num("EVR_WIDE16_ALT", 1);
    k.wide16_tail = num("EVR_WIDE16_TAIL", 1);
    if (const char* e = get("EVR_WIDE16_SHORT")) {
        if (!strcmp(e, "all")) k.wide16_short = WIDE16_SHORT_ALL;
        else if (!strncmp(e, "last=", 5)) { k.wide16_short = WIDE16_SHORT_LAST; k.wide16_short_last = atoi(e + 5) > 0 ? atoi(e + 5) : 0; }
        else k.wide16_short = atoi(e) != 0 ? WIDE16_SHORT_RULE : WIDE16_SHORT_OFF;
    }
    k.c16_blocks = num("EVR_C16_BLOCKS", 3);
    k.c16_out_nbuf = num("EVR_C16_OUT", 2); k.c16_out_blocks = second("EVR_C16_OUT", 3);
    k.c16_zr_nbuf = num("EVR_C16_ZR", 2); k.c16_zr_blocks = second("EVR_C16_ZR", 3);
    k.c16_rows = num("EVR_C16_ROWS", 1);
    k.c16_rows1_rows = num("EVR_C16_ROWS_1", 1); k.c16_rows1_blocks = second("EVR_C16_ROWS_1", 0);
    k.c16_rows2_rows = num("EVR_C16_ROWS_2", 2); k.c16_rows2_blocks = second("EVR_C16_ROWS_2", 0);
    k.lstm_dma = set("EVR_LSTM_DMA");
    k.lstm_wm8 = set("EVR_LSTM_WM8");
    return k;
}
const ConvKnobs& conv_knobs() {
    static const ConvKnobs k = conv_knobs_from([](const char* name) -> const char* { return getenv(name); });
    return k;
}

namespace {

// kw x kw taps in row-major order
bool taps_row_major(const ConvArgs& a, int kw) {
    for (int t = 0; t < kw * kw; ++t)
        if (a.tp.tap[t] != (((t / kw - kw / 2) & 0xffff) | ((t % kw - kw / 2) * 65536))) return false;
    return true;
}

// workspace of the split-K launches: ConvArgs::ksplit_ws, KSPLIT_WS_BYTES owned by the handle (model / LPIPS) whose plan this is --
// allocated with the plan, freed with it, never touched in the launch path (no hipMalloc / synchronisation here: a step can be
// captured into a hipGraph, and two devices or two handles never share partial sums)
bool ksplit_workspace_fits(const ConvArgs& a, size_t bytes) { return a.ksplit_ws && bytes <= KSPLIT_WS_BYTES; }

// the epilogue launch of a split-K convolution (ks runs per tile)
void route_ksplit_epilogue(ConvRoute& r, const ConvArgs& a, bool lstm, int total, const ConvKnobs& k) {
    const bool can4 = !(lstm && a.x3 == 4);      // (P6 tensors are written as whole 16-channel groups: the ConvLSTM quad form has no writer)
    r.epi_sum = 0; r.epi_grid = (unsigned)total;
    if (can4 && k.ksplit_epi4) {
        if (r.ks <= 4) { r.epi_sum = 4; r.epi_grid = (unsigned)(total * 4); }
        else if (r.ks <= KSPLIT_RUNS_MAX) { r.epi_sum = 8; r.epi_grid = (unsigned)(total * 4); }
        // (more runs than the wide form sums -- ksplit_cap never lets that happen -- fall through to the any-count epilogue)
    }
}

// conv3x3_band_kernel<4, 2, LSTM, GROUPED, false, PHASES>
ConvRoute route_band(ConvRoute r, const ConvArgs& a, bool lstm, bool grouped, int phases, const ConvKnobs& k) {
    constexpr int WM = 4;
    constexpr bool OVL = false;      // (the overlapped-tile form is gone; its tile width stays spelled out)
    const int M = a.n * a.hm * a.wm;
    const int tmv = OVL ? 32 * WM - 2 : 32 * WM;
    const int mtiles = (M + tmv - 1) / tmv;
    const int total = mtiles * (a.cout / 128);
    // split K when the launch leaves most of the 512 resident slots empty (small batches; the deep layers: a 346x260 sequence is 12
    // 128-pixel tiles at the bottom of the UNet) and K is long enough to cut: runs of >= 1 input-channel chunk, at most 4, never more
    // blocks than slots.  (A cost model that also split launches of 200-1000 tiles into more than one round measured slower: 1487 vs
    // 1599 frames/s at one sequence, 4098 vs 4356 at eight -- the partial accumulators are 64 KB per block each way.)
    int ks = 1;
    if (WM == 4 && !OVL) {
        const int ks_max = k.ksplit;      // (0 / 1: never)
        const int nchunks = (a.c0 + (a.in_mode == IN_CAT ? a.c1 : 0)) / 32;
        if (ks_max > 1 && total <= 192 && nchunks >= 2 && !a.pred_w) {
            ks = 512 / total;
            if (ks > nchunks) ks = nchunks;
            if (ks > k.ksplit_cap(total)) ks = k.ksplit_cap(total);
            if (ks < 2) ks = 1;
        }
    }
    if (ks > 1 && !ksplit_workspace_fits(a, (size_t)total * ks * 4 * 16 * 64 * sizeof(float4))) ks = 1;
    // (round 5: the 3-slot weight ring -- tiles requested TWO steps ahead, 84 KB of LDS -- for the split launches, which have one
    // block per CU and nobody to hide a DMA latency behind: 2095 vs 2206 frames/s at one sequence, 3856 vs 3944 at four.  Not kept.)
    r.family = CONV_BAND; r.wm = WM; r.lstm = lstm; r.grouped = grouped; r.phases = phases;
    r.grid = (unsigned)(total * ks); r.block = 64 * WM; r.lds = 0; r.ks = ks;
    if (ks > 1) route_ksplit_epilogue(r, a, lstm, total, k);
    return r;
}

// conv3x3_wide_kernel<LSTM, WN, GROUPED, PHASES> / conv3x3_wide16_kernel<WN, ALT, TAIL, SHORT> (SHORT and its grid: conv_route below)
ConvRoute route_wide(ConvRoute r, int family, const ConvArgs& a, bool lstm, int wn, bool grouped, int phases) {
    const int M = a.n * a.hm * a.wm;
    const int total = ((M + 255) / 256) * (a.cout / (128 * wn));
    r.family = family; r.lstm = lstm; r.wn = wn; r.grouped = grouped; r.phases = phases;
    r.grid = (unsigned)total; r.block = 256 * wn; r.lds = 0;
    return r;
}

// conv_igemm_kernel<KC, WM, NB, LSTM, GROUPED, REGSTAGE, X3>
ConvRoute route_igemm(ConvRoute r, const ConvArgs& a, int kc, int wm, int nb, bool lstm, bool grouped, bool regstage, int x3) {
    const int M = a.n * a.hm * a.wm;
    const int mtiles = (M + 32 * wm - 1) / (32 * wm);
    const int ntiles = a.cout / (32 * nb);
    const int total = mtiles * ntiles;
    r.family = CONV_IGEMM; r.kc = kc; r.wm = wm; r.nb = nb; r.lstm = lstm; r.grouped = grouped; r.regstage = regstage; r.x3 = x3;
    r.grid = (unsigned)total; r.block = 64 * wm; r.lds = 0;
    return r;
}

ConvRoute route_none(ConvRoute r, int err) { r.family = CONV_NONE; r.err = err; return r; }

// the band kernel takes: split arithmetic on PACKED inputs, 3x3 taps in row-major order, stride 1 on the input's own grid,
// N a multiple of 128, and enough pixels to fill the chip with 256-pixel tiles
bool band_eligible(const ConvArgs& a, int kc, const ConvKnobs& k) {
    if (k.no_band) return false;
    if (!(a.x3 && a.in_packed && kc == 32 && a.tp.ntaps == 9 && a.stride == 1)) return false;
    if (a.hm != a.hin || a.wm != a.win || a.cout % 128 != 0) return false;
    if (a.tp.ngroups == 1) { if (a.os != 1 || a.hout != a.hm || a.wout != a.wm) return false; }
    else if (a.os != 2 || a.hout != 2 * a.hm || a.wout != 2 * a.wm || a.epi == EPI_LSTM) return false;     // transposed conv
    if (!taps_row_major(a, 3)) return false;
    const int64_t M = (int64_t)a.n * a.hm * a.wm;
    // (round 3: no fill threshold any more -- for launches that do not fill the chip the band form still beats the implicit GEMM,
    // whose 9-fold A re-fetch is the cost either way: +16-17 % end to end at 1 / 4 / 8 / 16 sequences.  EVR_BAND_MIN restores one.)
    const int min_blocks = k.band_min;
    return ((M + 127) / 128) * (a.cout / 128) >= min_blocks;     // blocks of the default 128-pixel tiles
}

// split arithmetic on PACKED inputs, kw x kw taps in row-major order, stride 1 on the input's own grid; every epilogue but the
// ConvLSTM one (which needs 128-column tiles: conv3x3_band_kernel / conv3x3_wide_kernel).  kw = 5: the upsample-conv decoders;
// kw = 3: the 3x3 layers whose N is not a multiple of 128 (ConvGRU layouts, HyperE2VID's bases_net, FireNet padded to 32 channels)
bool bandk_eligible(const ConvArgs& a, int kc, int kw, const ConvKnobs& k) {
    if (!k.band5) return false;
    if (!(a.x3 && a.in_packed && kc == 32 && a.tp.ntaps == kw * kw && a.stride == 1 && a.tp.ngroups == 1) || a.no_band5) return false;
    if (a.hm != a.hin || a.wm != a.win || a.os != 1 || a.hout != a.hm || a.wout != a.wm || a.cout % 32 != 0) return false;
    if (a.epi == EPI_LSTM) return false;
    if (kw == 3 && a.cout % 128 == 0) return false;       // the 128-column kernels take those
    if (!taps_row_major(a, kw)) return false;
    const int nb = (a.cout % 128 == 0) ? 4 : (a.cout % 64 == 0) ? 2 : 1;
    if (a.pred_w && a.cout != 32 * nb) return false;      // a fused prediction needs a single N tile
    const int64_t M = (int64_t)a.n * a.hm * a.wm;
    const int min_blocks = k.band5_min;
    return ((M + 127) / 128) * (a.cout / (32 * nb)) >= min_blocks;
}

bool band_prog_eligible(const ConvArgs& a, int kc, const ConvKnobs& k) {
    if (k.no_band || !a.prog || !a.wgt2) return false;
    if (!(a.x3 && a.in_packed && kc == 32 && a.tp.ngroups == 1 && a.tp.ntaps == 25 && a.stride == 2 && a.os == 1)) return false;
    if (a.in_mode != IN_SINGLE || a.hin != 2 * a.hm || a.win != 2 * a.wm || a.hout != a.hm || a.wout != a.wm) return false;
    if (a.cout % 64 != 0 || a.pred_w) return false;
    // measured (64 sequences of 352x264): 64 columns (enc0) 595 -> 510 us with three bf16 products; at 128/256 columns the
    // band form only tied the implicit GEMM then, but with 2/3 of the matrix cycles the implicit GEMM's 25-fold A re-fetch
    // (64 B/clk/CU from L2) is the limit: 420/378 -> 395/360 us.  EVR_BAND_PROG_ALL=0 restores the implicit GEMM there.
    if (a.cout % 128 == 0 && !k.band_prog_all) return false;
    const int nb = (a.cout % 128 == 0) ? 4 : 2;
    const int64_t M = (int64_t)a.n * a.hm * a.wm;
    const int min_blocks = k.band_min;
    return ((M + 127) / 128) * (a.cout / (32 * nb)) >= min_blocks;
}

// conv_band_prog_kernel<NB> / conv_band_prog_wide_kernel<NB>
ConvRoute route_band_prog(ConvRoute r, const ConvArgs& a, int NB, const ConvKnobs& k) {
    const int M = a.n * a.hm * a.wm;
    const int total = ((M + 127) / 128) * (a.cout / (32 * NB));
    int ks = 1;
    if (NB == 4) {      // split K for under-filled launches (launch_band's rule; runs are whole bands of the step program)
        const int ks_max = k.ksplit;
        const int nbands = a.prog_steps / 2;      // (>= 2 steps per band on average: an upper bound that keeps every run non-empty)
        if (ks_max > 1 && total <= 192 && nbands >= 4) {
            ks = 512 / total;
            if (ks > nbands / 2) ks = nbands / 2;
            if (ks > k.ksplit_cap(total)) ks = k.ksplit_cap(total);
            if (ks < 2) ks = 1;
        }
    }
    r.nb = NB; r.block = 256; r.lds = 0;
    {   // 256-pixel tiles once a launch has enough of them to fill the chip (two or three blocks per CU; EVR_PROG_WIDE=0: never)
        const int total2 = ((M + 255) / 256) * (a.cout / (32 * NB));
        if (k.prog_wide && total2 >= k.prog_wide_min && ks == 1) {
            r.family = CONV_BAND_PROG_WIDE; r.grid = (unsigned)total2;
            return r;
        }
    }
    if (ks > 1 && !ksplit_workspace_fits(a, (size_t)total * ks * 4 * 16 * 64 * sizeof(float4))) ks = 1;
    if (NB == 4 && ks > 1) {
        r.family = CONV_BAND_PROG_KSPLIT; r.grid = (unsigned)(total * ks); r.ks = ks;
        route_ksplit_epilogue(r, a, false, total, k);
        return r;
    }
    r.family = CONV_BAND_PROG; r.grid = (unsigned)total;
    return r;
}

// rows per segment: about two items per resident block, even, at least 8 (the halo rows are fetched once more per segment)
void c16_rows_plan(const ConvArgs& a, int blocks, int* rseg, int* nseg, int* nstrips) {
    const int H = a.hin, W = a.win;
    *nstrips = (W + 127) / 128;
    int want = (2 * blocks + a.n * *nstrips - 1) / (a.n * *nstrips);
    if (want < 1) want = 1;
    int rs = (H + want - 1) / want;
    rs = (rs + 1) & ~1;
    if (rs < 8) rs = 8;
    *rseg = rs; *nseg = (H + rs - 1) / rs;
}

// EVR_C16_ROWS: 0 = the tile kernel everywhere, 2 = the row kernel whatever the size
bool c16_rows_eligible(const ConvArgs& a, const ConvKnobs& k) {
    if (k.c16_rows <= 0) return false;
    if ((int64_t)a.n * a.hin * a.win >= (1LL << 26)) return false;      // (32-bit byte offsets of 64-B pixels)
    if ((a.epi == EPI_GRU_ZR || a.epi == EPI_GRU_OUT) && a.hidden != 16) return false;      // (gru_prefetch16)
    // (a small batch has too few (strip, segment) items to fill the chip: the tile kernel's 128-pixel tiles stay; EVR_C16_ROWS=2
    // lifts the threshold -- the parity tests' small shapes)
    return k.c16_rows >= 2 || (int64_t)a.n * ((a.win + 127) / 128) * ((a.hin + 7) / 8) >= 1024;
}

// conv3x3_c16_rows_kernel<1, RPB, NSRC, HALFW>
ConvRoute route_c16_rows(ConvRoute r, const ConvArgs& a, const ConvKnobs& k) {
    constexpr int NB = 1;
    const int nsrc = (a.in_mode == IN_CAT && a.c1) ? 2 : 1;
    const bool half_w = NB == 1 && a.n_valid <= 16;
    // rows per step and blocks per CU: EVR_C16_ROWS_1=<rows>,<blocks> for the one-source layers, EVR_C16_ROWS_2 for the two-source ones
    // (A/B).  LDS: one source, 1 row = 4 x 8.3 + 18 (9) KB -> three blocks; two sources, 2 rows = 12 x 8.3 + 36 (18) KB -> one block of 8 waves
    const int rows = nsrc == 1 ? k.c16_rows1_rows : 2, bl = nsrc == 1 ? k.c16_rows1_blocks : k.c16_rows2_blocks;      // (two sources: always two rows per step -- one row per step leaves four waves on the CU)
    const int per_cu = bl > 0 ? bl : (rows == 2 ? 1 : (nsrc == 1 ? 3 : 1));
    const int RPB = rows == 2 ? 2 : 1, NSRC = rows == 2 ? nsrc : 1;      // (the one-row form exists for one source only)
    const int NBUF = 2 * RPB + 2;
    const int wrows = half_w ? 16 : 32 * NB;
    const size_t lds_bytes = ((size_t)NSRC * NBUF * (128 + 2) * 4 + (size_t)9 * NSRC * wrows * 4 + 4 + 8 * NB) * sizeof(float4);
    const int ntiles_n = a.cout / (32 * NB);
    int rseg, nseg, nstrips;
    c16_rows_plan(a, 256 * per_cu, &rseg, &nseg, &nstrips);
    int64_t items = (int64_t)a.n * nseg * nstrips;
    int blocks = 256 * per_cu;
    if (blocks > items) blocks = (int)items;
    r.family = CONV_C16_ROWS; r.nb = NB; r.rpb = RPB; r.nsrc = NSRC; r.halfw = half_w; r.nbuf = NBUF;
    r.grid = (unsigned)(blocks * ntiles_n); r.block = 256 * RPB; r.lds = lds_bytes;
    r.rseg = rseg; r.nseg = nseg; r.nstrips = nstrips;
    return r;
}

// conv3x3_c16_kernel<1, NBUF>
ConvRoute route_c16_tile(ConvRoute r, const ConvArgs& a, const ConvKnobs& k) {
    constexpr int NB = 1;
    const int M = a.n * a.hm * a.wm;
    const int mtiles = (M + 127) / 128, ntiles_n = a.cout / (32 * NB);
    const int nsrc = (a.in_mode == IN_CAT && a.c1) ? 2 : 1;
    // SHIPPED DEFAULTS: two band buffers and three blocks per CU for every layer.  One-source layers (residual convolutions): measured
    // 3 > 4 > 2 blocks (157 / 183 / 189 us); two-source layers (ConvGRU z|r gates, 32 real columns; the candidate convolution, <= 16
    // real columns = half the weight rows): three blocks with two buffers beat the ring of four at two blocks (273 vs 312-320 us,
    // 265 vs 308-381).  EVR_C16_ZR / EVR_C16_OUT=<nbuf>,<blocks> select the ring of four (nbuf = 4, 70 KB) for A/B runs.
    const bool half_w = NB == 1 && a.n_valid <= 16;
    const int nbuf = nsrc == 1 ? 2 : (half_w ? (k.c16_out_nbuf == 4 ? 4 : 2) : (k.c16_zr_nbuf == 4 ? 4 : 2));
    const int wrows = half_w ? 16 : 32 * NB;
    const size_t lds_bytes = ((size_t)nbuf * (128 + 2) * 4 + (size_t)9 * nsrc * wrows * 4 + 4) * sizeof(float4);
    int per_cu = nsrc == 1 ? (k.c16_blocks > 0 ? k.c16_blocks : 3) : (half_w ? (k.c16_out_blocks > 0 ? k.c16_out_blocks : 3) : (k.c16_zr_blocks > 0 ? k.c16_zr_blocks : 3));
    int per_n = 256 * per_cu;                             // persistent: the resident blocks walk the M tiles
    if (per_n > mtiles) per_n = mtiles;
    r.family = CONV_C16_TILE; r.nb = NB; r.nsrc = nsrc; r.halfw = half_w; r.nbuf = nbuf;
    r.grid = (unsigned)(per_n * ntiles_n); r.block = 256; r.lds = lds_bytes;
    return r;
}

}  // namespace

bool conv_c16_eligible(const ConvArgs& a, int kc) {
    if (!(a.x3 == 3 && a.in_packed && kc == 16 && a.tp.ntaps == 9 && a.stride == 1 && a.tp.ngroups == 1)) return false;
    if (a.c0 != 16 || !(a.in_mode == IN_SINGLE || a.c1 == 16)) return false;
    if (a.hm != a.hin || a.wm != a.win || a.os != 1 || a.hout != a.hm || a.wout != a.wm || a.cout != 32) return false;      // (one N tile of 32 columns: every FireNet layer)
    if (a.epi == EPI_LSTM) return false;
    return taps_row_major(a, 3);
}

ConvRoute conv_route(const ConvArgs& a, int kc, int wm, int nb, const ConvKnobs& k) {
    ConvRoute r = {};
    r.ks = 1;
    const bool mx_object = a.x3 != 3 && a.x3 != 4;      // conv.hip's mode-2 object: it alone carries the exact-fp32 (X3 = 0) kernels
    if (conv_c16_eligible(a, kc)) {
        if (c16_rows_eligible(a, k)) return route_c16_rows(r, a, k);
        return route_c16_tile(r, a, k);
    }
    const int mode = a.x3 ? 2 : 0;
    if (band_prog_eligible(a, kc, k)) return route_band_prog(r, a, a.cout % 128 == 0 ? 4 : 2, k);
    if (const int kw = bandk_eligible(a, kc, 5, k) ? 5 : (bandk_eligible(a, kc, 3, k) ? 3 : 0)) {
        const int NB = (kw == 5 && a.cout % 128 == 0) ? 4 : (a.cout % 64 == 0) ? 2 : 1;
        const int M = a.n * a.hm * a.wm;
        const int total = ((M + 127) / 128) * (a.cout / (32 * NB));
        // (a.band_lds_pad: extra dynamic LDS per block -- caps the blocks a CU holds, for launches that share the chip with another stream)
        r.family = CONV_BANDK; r.kw = kw; r.nb = NB; r.grid = (unsigned)total; r.block = 256; r.lds = (size_t)a.band_lds_pad;
        return r;
    }
    if (band_eligible(a, kc, k)) {
        // 128 x 128 tiles: 4 waves x 2-slot ring, two blocks per CU (one block's epilogue and barrier bubbles hide under the
        // other's MFMAs).  The 8-wave and overlapped-tile / 3-slot-ring configurations of earlier rounds measured slower
        // (profiles/r02_tile_variants.txt) and are gone: with the zero row their 80 KiB no longer leave two blocks per CU.
        // 256-pixel block tiles when N allows and there are enough of them to fill the chip (EVR_WIDE=0: never)
        const int wide = k.wide;
        const int wide_min = k.wide_min;
        // two 256 x 128 blocks per CU (one band buffer each) while K is short, one 256 x 256 block otherwise: measured
        // 1486 / 1449 / 1405 us against 1585 / 1489 / 1401 us for 128 / 256 / 512 input channels (EVR_WIDE=2 / 3 force one)
        // (round 8, the 256 x 256 form on its skewed loop, 64 sequences, two-stream step, us per launch enc0 / enc1 / enc2.rec: this rule
        // 1885 / 1822 / 1708 and 1925 / 1850 / 1703, EVR_WIDE=3 1855 / 1803 / 1696 and 1879 / 1810 / 1706, EVR_WIDE=3 on the lock-step
        // loop 1991 / 1904 / 1790 and 2040 / 1953 / 1849.  The 256 x 256 form now leads on the short-K layers too, by 1-2 %; the rule
        // stays until the tile-count thresholds below, taken on the lock-step loop, are measured again at 4 - 32 sequences)
        // (round 9, measured again on the skewed loop with the trimmed tail, us per launch twin / 256 x 256, single-stream step,
        // profiles/r09_layer_times.txt: enc0.rec -- 128 input channels -- 5808 tiles 1852 / 1822, 2904 tiles 902 / 915, 1452 tiles 471 / 454,
        // 726 tiles 240 / 235; enc1.rec -- 256 channels -- 2904 tiles 1841 / 1800, 1452 tiles 890 / 852, 726 tiles 447 / 422.  From the
        // 256 x 256 form's own threshold on the short-K layers take it too, with one exception that keeps the twin form: 128 channels and
        // a last round of 256 blocks less than half full (2904 = 11.34 rounds), which the twin form's 512 half-width slots finish in
        // finer pieces.  Below that threshold, and with an explicit EVR_WIDE_MIN, the rule is what it was)
        const int64_t wide_tiles = (((int64_t)a.n * a.hm * a.wm + 255) / 256) * (a.cout / 256);
        const bool ragged = wide_tiles % 256 != 0 && wide_tiles % 256 < 128;
        const bool short_k_twin = k.wide_min_set || wide_tiles < wide_min || (a.c0 + a.c1 <= 128 && ragged);
        const bool twin = (wide == 2) || (wide == 1 && a.c0 + a.c1 <= 256 && short_k_twin);
        // (the twin form already pays from ~1.4 rounds of its 512 slots on: per-layer times at 4 / 8 sequences, enc0.rec 144 -> 138 us
        // with 726 twin tiles, enc1.rec 262 -> 249 us with 728; below one round it loses -- enc1.rec 136 -> 151 us with 364 tiles -- and
        // the 256 x 256 form loses up to its own threshold: enc2.rec 256 -> 279 us at 8 sequences.  Explicit EVR_WIDE_MIN: one threshold)
        const int wide_min_twin = k.wide_min_twin;
        const bool wide_ok = wide && a.tp.ngroups == 1 && a.cout % 256 == 0 && !a.pred_w &&
                             (((int64_t)a.n * a.hm * a.wm + 255) / 256) * (a.cout / 256) >= (twin ? wide_min_twin : wide_min);
        if (wide_ok && a.epi == EPI_LSTM) {
            if (a.x3 == 3) {      // (h3 object only)
                // the same tiles on 16x16x32 MFMAs (conv3x3_wide16_kernel); EVR_MFMA16=0: the 32x32x16 form
                // the 256 x 256 form runs its skewed loop (wave halves alternate load and MFMA); EVR_WIDE16_ALT=0: the lock-step loop
                if (k.mfma16) {
                    r = route_wide(r, CONV_WIDE16, a, true, twin ? 1 : 2, false, 0);
                    r.alt = !twin && k.wide16_alt;
                    // the trimmed prologue / epilogue (TAIL, above the kernel); EVR_WIDE16_TAIL=0: the tile's fixed part as it was
                    r.tail = k.wide16_tail != 0;
                    // 192-pixel tiles in the ragged last round: the plan's map (conv_plan_wide16_map below; EVR_WIDE16_SHORT=0: never one)
                    r.short16 = r.alt && r.tail && a.w16map.slots > 0;
                    if (r.short16) r.grid = 8u * (unsigned)a.w16map.slots * (unsigned)(a.cout / 256);
                    return r;
                }
            }
            return route_wide(r, CONV_WIDE, a, true, twin ? 1 : 2, false, 0);
        }
        // plain 3x3 layers (residual blocks): the twin form once a launch has enough 256 x 128 tiles (not at 64 sequences of
        // 346x260: 726 tiles for 512 slots; from 128 sequences or 640x480 up)
        // (their own threshold: at 64 sequences the residual convolutions are 726 such tiles -- 1.42 rounds of 512 slots -- and run
        // 281 us on this form against 258 us on the 128 x 128 tiles; the ConvLSTM threshold above went down to 600 in round 5)
        const int wide_min_plain = k.wide_min_plain;
        if (wide && a.tp.ngroups == 1 && a.cout % 128 == 0 && !a.pred_w &&
            (a.epi == EPI_BIAS || a.epi == EPI_BIAS_RELU || a.epi == EPI_RESIDUAL_RELU) &&
            (((int64_t)a.n * a.hm * a.wm + 255) / 256) * (a.cout / 128) >= wide_min_plain)
            return route_wide(r, CONV_WIDE, a, false, 1, false, 0);
        if (a.epi == EPI_LSTM) {
            return route_band(r, a, true, false, 0, k);
        }
        if (a.tp.ngroups > 1) {
            // does the tap/phase connectivity follow the k5 s2 p2 rule the PHASES variants compile in?
            bool rule = a.tp.ngroups == 4;
            for (int t = 0; t < 9 && rule; ++t) {
                int want = 0;
                for (int g = 0; g < 4; ++g) if (!((g >> 1) == 1 && t / 3 == 0) && !((g & 1) == 1 && t % 3 == 0)) want |= 1 << g;
                rule = a.tp.tap_groups[t] == want;
            }
            for (int g = 0; g < 4 && rule; ++g) rule = a.tp.grp_ofy[g] == (g >> 1) && a.tp.grp_ofx[g] == (g & 1);
            // 256 x 128 tiles, two blocks per CU (the twin form of conv3x3_wide_kernel), once there are enough of them:
            // half the LDS-DMA bytes per MFMA cycle of the 128 x 128 tiles (EVR_WIDE_DEC=0: never)
            const int wide_dec = k.wide_dec;
            // (dec2 -- 32 output channels, 18 steps -- gains from 363 such tiles on: 49 -> 39 us at 4 sequences; dec1 at 364 loses, 83 -> 92 us)
            const int wide_min_dec32 = k.wide_min_dec32;
            const bool twin_ok = wide_dec && rule && (((int64_t)a.n * a.hm * a.wm + 255) / 256) * (a.cout / 128) >= (a.tp.grp_cols == 32 ? wide_min_dec32 : wide_min) &&
                                 (a.epi == EPI_BIAS || a.epi == EPI_BIAS_RELU) && (!a.pred_w || a.tp.grp_cols == 32);   // (a fused
            // prediction must close inside one 32-column block: the epilogue runs block by block)
            if (twin_ok && a.tp.grp_cols == 32) return route_wide(r, CONV_WIDE, a, false, 1, true, 1);
            if (twin_ok && a.tp.grp_cols == 64) return route_wide(r, CONV_WIDE, a, false, 1, true, 2);
            if (twin_ok && a.tp.grp_cols % 128 == 0) return route_wide(r, CONV_WIDE, a, false, 1, true, 0);
            if (rule && a.tp.grp_cols == 32) return route_band(r, a, false, true, 1, k);
            if (rule && a.tp.grp_cols == 64) return route_band(r, a, false, true, 2, k);
            return route_band(r, a, false, true, 0, k);
        }
        return route_band(r, a, false, false, 0, k);
    }
    const bool wmnb = (wm == 4 || wm == 2 || wm == 1) && (nb == 4 || nb == 2 || nb == 1);      // the tiles the non-LSTM implicit GEMM is built with
    if (a.epi == EPI_LSTM) {
        if (kc != 32) return route_none(r, ROUTE_LSTM_KC);
        if (mode == 2) {
            if (wm == 8) return route_igemm(r, a, 32, 8, 4, true, false, true, 2);
            if (wm == 4) return route_igemm(r, a, 32, 4, 4, true, false, true, 2);
            if (wm == 2) return route_igemm(r, a, 32, 2, 4, true, false, false, 2);
            return route_igemm(r, a, 32, 1, 4, true, false, false, 2);
        }
        if (mx_object) {
            if (wm == 8) return route_igemm(r, a, 32, 8, 4, true, false, false, 0);
            // register staging measured +1..4 % over LDS-DMA for this kernel (EVR_LSTM_DMA=1 selects the DMA loader)
            if (wm == 4 && !k.lstm_dma) return route_igemm(r, a, 32, 4, 4, true, false, true, 0);
            if (wm == 4) return route_igemm(r, a, 32, 4, 4, true, false, false, 0);
            if (wm == 2) return route_igemm(r, a, 32, 2, 4, true, false, false, 0);
            return route_igemm(r, a, 32, 1, 4, true, false, false, 0);
        }
    }
    if (a.tp.ngroups > 1) {   // transposed conv: column groups = sub-pixel phases
        if (kc == 32 && wmnb) return route_igemm(r, a, 32, wm, nb, false, true, false, (mx_object && mode != 2) ? 0 : 2);
        return route_none(r, ROUTE_NO_GROUPED);
    }
    if (mode != 0 && wmnb) return route_igemm(r, a, 32, wm, nb, false, false, false, 2);
    if (mx_object && wmnb && (kc == 32 || (kc == 16 && nb == 1))) return route_igemm(r, a, kc, wm, nb, false, false, false, 0);
    return route_none(r, ROUTE_NO_KERNEL);
}

// ---------------------------------------------------------------------------------------------------
// The tile map of conv3x3_wide16_kernel<2, true, true>.  The form holds ONE block per CU and its tiles are all alike, so a launch of T
// tiles on C units takes ceil(T / C) rounds however empty the last one is (profiles/r10_tail_pricing.txt: 5.50, 5.67 and 5.95 rounds cost
// the same).  The mixed map spends the same whole number of rounds R on R * C blocks instead: as many 256-pixel tiles as before minus the
// ones that four 192-pixel tiles replace three of, so that the last round is full and part of the blocks finish early everywhere.
namespace {

// `slots` places per XCD range, the last shorts[x] of them 192 pixels: walk the M pixels through the ranges in order
Wide16Map fill_ranges(int64_t M, int slots, const int (&shorts)[8]) {
    Wide16Map m = {};
    m.slots = slots;
    int64_t pix = 0;
    for (int x = 0; x < 8; ++x) {
        m.pix0[x] = (int)pix;
        int64_t nf = (M - pix + 255) / 256;
        if (nf > slots - shorts[x]) nf = slots - shorts[x];
        pix = pix + 256 * nf < M ? pix + 256 * nf : M;
        int64_t ns = (M - pix + 191) / 192;
        if (ns > shorts[x]) ns = shorts[x];
        pix = pix + 192 * ns < M ? pix + 192 * ns : M;
        m.full[x] = (int)nf; m.count[x] = (int)(nf + ns);
    }
    return m;      // (pix == M when the capacity of the ranges covers M: the callers see to that)
}

}  // namespace

double wide16_makespan(const Wide16Map& m, int nt, int cus_per_xcd, double rho) {
    double worst = 0.0;
    std::vector<double> free_at((size_t)(cus_per_xcd > 0 ? cus_per_xcd : 1));
    for (int x = 0; x < 8; ++x) {
        std::fill(free_at.begin(), free_at.end(), 0.0);
        for (int t = 0; t < m.count[x]; ++t)
            for (int j = 0; j < nt; ++j) {
                auto cu = std::min_element(free_at.begin(), free_at.end());
                *cu += t < m.full[x] ? 1.0 : rho;
            }
        const double end = *std::max_element(free_at.begin(), free_at.end());
        if (end > worst) worst = end;
    }
    return worst;
}

Wide16Plan wide16_tile_map(int64_t M, int nt, int cus, int mode, int last_k) {
    Wide16Plan p = {};
    p.mtiles = (int)((M + 255) / 256);
    if (M <= 0 || nt <= 0 || mode == WIDE16_SHORT_OFF) return p;
    int shorts[8];
    if (mode == WIDE16_SHORT_ALL) {
        const int slots = (int)(((M + 191) / 192 + 7) / 8);
        for (int& s : shorts) s = slots;
        p.map = fill_ranges(M, slots, shorts);
    } else if (mode == WIDE16_SHORT_LAST) {
        int slots = 1;
        const auto cap = [&](int sl) { const int s = last_k < sl ? last_k : sl; return 8 * (256LL * (sl - s) + 192LL * s); };
        while (cap(slots) < M) ++slots;
        for (int& s : shorts) s = last_k < slots ? last_k : slots;
        p.map = fill_ranges(M, slots, shorts);
    } else {
        // the rule: the smallest whole number of rounds R whose R * cus blocks -- Mt = R * cus / nt M tiles of at most 256 pixels, the same
        // number in every XCD range -- cover M; then b tiles can give up 64 pixels each
        if (cus <= 0 || cus % (8 * nt) != 0) return p;
        const int64_t per_round = cus / nt;
        const int64_t R = (M + 256 * per_round - 1) / (256 * per_round), Mt = R * per_round;
        int64_t b = (256 * Mt - M) / 64;
        if (b > Mt) b = Mt;
        // (nothing to give up; or M so small that even 192-pixel tiles leave some of the Mt without a pixel: the uniform map)
        if (b == 0 || 256 * (Mt - b) + 192 * b - M >= 192 || Mt * nt > (1LL << 30)) return p;
        for (int x = 0; x < 8; ++x) shorts[x] = (int)(b / 8 + (x < b % 8 ? 1 : 0));
        const Wide16Map m = fill_ranges(M, (int)(Mt / 8), shorts);
        // whole rounds of the uniform map (its XCD ranges hold total / 8 blocks, the first total % 8 of them one more)
        const int64_t total = (int64_t)p.mtiles * nt;
        p.makespan_uniform = (double)(((total + 7) / 8 + cus / 8 - 1) / (cus / 8));
        p.makespan = wide16_makespan(m, nt, cus / 8, WIDE16_SHORT_RHO);
        if (!(p.makespan <= p.makespan_uniform - WIDE16_SHORT_MARGIN)) return p;
        p.map = m;
    }
    p.mtiles = 0; p.nshort = 0;
    for (int x = 0; x < 8; ++x) { p.mtiles += p.map.count[x]; p.nshort += p.map.count[x] - p.map.full[x]; }
    return p;
}

void conv_plan_wide16_map(ConvArgs& a, int kc, int wm, int nb, int cus, const ConvKnobs& k) {
    a.w16map = {};
    if (k.wide16_short == WIDE16_SHORT_OFF) return;
    const ConvRoute r = conv_route(a, kc, wm, nb, k);
    if (r.family != CONV_WIDE16 || r.wn != 2 || !r.alt || !r.tail) return;
    // (the rule keeps clear of everything an explicit EVR_WIDE_MIN moves: the shapes the tests pin run the map they always had)
    if (k.wide16_short == WIDE16_SHORT_RULE && k.wide_min_set) return;
    a.w16map = wide16_tile_map((int64_t)a.n * a.hm * a.wm, a.cout / 256, cus, k.wide16_short, k.wide16_short_last).map;
}

}  // namespace evr
