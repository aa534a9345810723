// Which kernel a convolution launch gets (host only): the table of run-time switches of the conv dispatch, read once, and the pure
// function from a launch plan to a launch description.  conv.hip's launch_conv_igemm_* validate the plan, ask conv_route() and
// launch what it names; nothing here calls HIP, allocates or keeps state (conv_knobs()'s one table apart).
#pragma once
#include "conv.h"

namespace evr {

constexpr int KSPLIT_RUNS_MAX = 8;      // what conv_ksplit_epi4_kernel<..., 8> sums; ksplit_cap clamps EVR_KSPLIT / EVR_KSPLIT_SMALL to it
enum Wide16ShortMode { WIDE16_SHORT_OFF = 0, WIDE16_SHORT_RULE = 1, WIDE16_SHORT_ALL = 2, WIDE16_SHORT_LAST = 3 };

// Every switch of the conv dispatch (README "Run-time switches" lists them in this order).  Fields hold the values in force:
// defaults that depend on another switch being set are resolved where the table is filled (conv_knobs_from).
struct ConvKnobs {
    // ---- which family takes a layer
    bool no_band = false;         // EVR_NO_BAND (set, any value): no band kernel of any kind -- the implicit GEMM everywhere
    int band_min = 1;             // EVR_BAND_MIN: fewest 128-pixel blocks for the 3x3 and programmed band forms (no fill threshold since round 3)
    bool band5 = true;            // EVR_BAND5=0 (or EVR_NO_BAND): no k x k band form (conv_bandk_kernel)
    int band5_min = 1;            // EVR_BAND_MIN if set, else EVR_BAND5_MIN: fewest blocks for the k x k band form
    bool band_prog_all = true;    // EVR_BAND_PROG_ALL=0: the k5 s2 encoders of 128 / 256 columns stay on the implicit GEMM
    int prog_wide = 1;            // EVR_PROG_WIDE=0: the programmed band kernel never takes 256-pixel tiles
    int prog_wide_min = 600;      // EVR_PROG_WIDE_MIN: fewest 256-pixel tiles for that form
    // ---- split K (launch_band's rule, also the programmed band kernel's)
    int ksplit = 4;               // EVR_KSPLIT: most runs per tile (0 / 1: never)
    int ksplit_small = 8;         // EVR_KSPLIT_SMALL: most runs for launches of <= 64 tiles; default EVR_KSPLIT set ? 0 : 8
    int ksplit_epi4 = 1;          // EVR_KSPLIT_EPI4 (A/B: 0 = one block per tile)
    // ---- 256-pixel tiles of the 3x3 band layers
    int wide = 1;                 // EVR_WIDE: 0 never, 2 / 3 force the twin / the 256 x 256 form
    int wide_min = 600;           // EVR_WIDE_MIN (round 5: 600 tiles, was 1024 -- +2 % at 8 / 16 / 32 sequences, equal at 4 and 64; 300: -1 % at 16 / 32.  Tests lower it)
    bool wide_min_set = false;    //   set explicitly: one threshold -- it also replaces the three below and the ragged-round rule
    int wide_min_twin = 350;      //   the twin ConvLSTM form's own threshold
    int wide_min_dec32 = 350;     //   the 32-column transposed decoder's (dec2)
    int wide_min_plain = 1024;    // EVR_WIDE_MIN_PLAIN: the plain 3x3 layers' (residual blocks); overrides only this one
    int wide_dec = 1;             // EVR_WIDE_DEC=0: the transposed decoders never take the twin form
    int mfma16 = 1;               // EVR_MFMA16=0: the ConvLSTM gate launches on the 32x32x16 form (h3 object)
    int wide16_alt = 1;           // EVR_WIDE16_ALT=0: the 256 x 256 16x16x32 form on its lock-step loop
    int wide16_tail = 1;          // EVR_WIDE16_TAIL=0: the tile's fixed part as it was (no trimmed prologue / epilogue)
    int wide16_short = WIDE16_SHORT_RULE;   // EVR_WIDE16_SHORT: 0 never a 192-pixel tile (A/B), unset / 1 the rule of wide16_tile_map, "all" every tile
    int wide16_short_last = 0;    //   short, "last=<k>" the last k M tiles of every XCD range short (the last two: tests, and measuring a short tile)
    // ---- FireNet's 16-channel layers (h3 object)
    int c16_blocks = 3;           // EVR_C16_BLOCKS (A/B: blocks per CU of the one-source form)
    int c16_out_nbuf = 2, c16_out_blocks = 3;     // EVR_C16_OUT=<nbuf>,<blocks>: the candidate convolution (nbuf 4 = the ring of four)
    int c16_zr_nbuf = 2, c16_zr_blocks = 3;       // EVR_C16_ZR=<nbuf>,<blocks>: the z|r gate launches
    int c16_rows = 1;             // EVR_C16_ROWS: 0 = the tile kernel everywhere, 2 = the row kernel whatever the size
    int c16_rows1_rows = 1, c16_rows1_blocks = 0; // EVR_C16_ROWS_1=<rows>,<blocks>: rows per step and blocks per CU, one-source layers (A/B; 0 blocks: by LDS)
    int c16_rows2_rows = 2, c16_rows2_blocks = 0; // EVR_C16_ROWS_2=<rows>,<blocks>: two-source layers.  The row count is parsed and NOT used: always two rows per step
    // ---- implicit GEMM
    bool lstm_dma = false;        // EVR_LSTM_DMA (set): the fp32 ConvLSTM kernel at WM = 4 on the DMA loader, not register staging
    bool lstm_wm8 = false;        // EVR_LSTM_WM8 (set): pick_conv_tile gives the ConvLSTM a 256x128 block tile (experiment)

    // most runs per tile: 4, and 8 for launches of at most 64 tiles (the residual convolutions and dec0 of ONE sequence: 24 / 48 tiles --
    // eight runs still leave slots free).  Measured on one box, three runs each, +-0.1 %: a flat cap of 8 is +1.1 % at one sequence (2183 vs
    // 2159 frames/s) and -1.0 % at four (5 runs for the 92-tile residual convolutions and enc2.rec: the 8-run epilogue kernel holds one block
    // per CU); caps of 5 / 6: -3 % at one sequence; 5-6 runs for 65-102 tiles with a six-run epilogue kernel at two blocks per CU: 2206 vs 2245 at
    // one sequence, equal at four.  EVR_KSPLIT sets the general cap, EVR_KSPLIT_SMALL the one for <= 64 tiles.
    // Both switches are clamped to KSPLIT_RUNS_MAX = 8: conv_ksplit_epi4_kernel<..., 8> sums at most eight partial sets (with
    // EVR_KSPLIT=16 the main kernel wrote sixteen and the epilogue silently summed the first eight).
    int ksplit_cap(int total) const {
        const int cap = (total <= 64 && ksplit_small > ksplit) ? ksplit_small : ksplit;
        return cap > KSPLIT_RUNS_MAX ? KSPLIT_RUNS_MAX : cap;
    }
};
// the table for a given environment (`get`: getenv or a stand-in), and the process's own, filled on first use
ConvKnobs conv_knobs_from(const char* (*get)(const char*));
const ConvKnobs& conv_knobs();

enum ConvFamily {
    CONV_NONE = 0,          // no kernel: ConvRoute::err says which message
    CONV_C16_TILE,          // conv3x3_c16_kernel<1, NBUF>
    CONV_C16_ROWS,          // conv3x3_c16_rows_kernel<1, RPB, NSRC, HALFW>
    CONV_BAND_PROG,         // conv_band_prog_kernel<NB, false>: 128-pixel tiles
    CONV_BAND_PROG_WIDE,    // conv_band_prog_wide_kernel<NB>: 256-pixel tiles
    CONV_BAND_PROG_KSPLIT,  // conv_band_prog_kernel<4, true> + the split-K epilogue
    CONV_BANDK,             // conv_bandk_kernel<KW, NB>
    CONV_BAND,              // conv3x3_band_kernel<4, 2, LSTM, GROUPED, false, PHASES, ks > 1> (+ the split-K epilogue)
    CONV_WIDE,              // conv3x3_wide_kernel<LSTM, WN, GROUPED, PHASES>
    CONV_WIDE16,            // conv3x3_wide16_kernel<WN, ALT, TAIL, SHORT>
    CONV_IGEMM              // conv_igemm_kernel<KC, WM, NB, LSTM, GROUPED, REGSTAGE, X3>
};
enum ConvRouteErr { ROUTE_OK = 0, ROUTE_LSTM_KC, ROUTE_NO_GROUPED, ROUTE_NO_KERNEL };
struct ConvRoute {
    int family, err;
    // template selectors (those of `family` are meaningful)
    int kc, wm, nb, x3, phases, wn, kw, rpb, nsrc, nbuf;
    bool lstm, grouped, regstage, alt, tail, halfw;
    bool short16;                   // CONV_WIDE16: the plan carries a tile map (ConvArgs::w16map) -- the grid is the map's, the kernel the SHORT one
    unsigned grid, block;
    size_t lds;                     // dynamic LDS bytes
    int ks;                         // split-K runs per tile (1: no split, no epilogue launch)
    int epi_sum;                    // ks > 1: conv_ksplit_epi4_kernel<..., 4 | 8>, or 0: conv_ksplit_epilogue_kernel
    unsigned epi_grid;
    int rseg, nseg, nstrips;        // CONV_C16_ROWS: the kernel's segment arguments
};

bool conv_c16_eligible(const ConvArgs& a, int kc);
ConvRoute conv_route(const ConvArgs& a, int kc, int wm, int nb, const ConvKnobs& k);

// ---- the tile map of the skewed 256 x 256 ConvLSTM form (conv3x3_wide16_kernel<2, true, true>): 192-pixel tiles fill the ragged last round
// A 192-pixel tile's time in units of a 256-pixel tile's (profiles/r10_layer_times.txt, section B: every tile forced short at 55
// sequences, where both maps fill their rounds -- 0.787 / 0.791 / 0.767 on enc0 / enc1 / enc2.rec), and how many full-tile times the
// mixed map's predicted makespan must lie below the uniform map's whole rounds before a launch takes it
constexpr double WIDE16_SHORT_RHO = 0.79;
constexpr double WIDE16_SHORT_MARGIN = 0.15;
struct Wide16Plan {
    Wide16Map map;                  // slots == 0: the uniform map
    int mtiles, nshort;             // M tiles in all, and how many of them are 192 pixels
    double makespan, makespan_uniform;      // predicted, in full-tile times (rule mode only)
};
// M pixels, nt N tiles per M tile, `cus` compute units (one block each); mode / last_k: ConvKnobs::wide16_short / wide16_short_last
Wide16Plan wide16_tile_map(int64_t M, int nt, int cus, int mode, int last_k);
// blocks of one XCD range handed in grid order to cus_per_xcd units, a full tile 1 and a short one rho: when the last one ends
double wide16_makespan(const Wide16Map& m, int nt, int cus_per_xcd, double rho);
// plan time: a.w16map for the launch conv_route() gives this plan (none unless it is the skewed form with the trimmed tail; the rule
// also leaves launches under an explicit EVR_WIDE_MIN alone).  conv_route() then reads the map back from the plan
void conv_plan_wide16_map(ConvArgs& a, int kc, int wm, int nb, int cus, const ConvKnobs& k);

}  // namespace evr
