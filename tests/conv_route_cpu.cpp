// Stand-alone host program of tests/test_conv_route_cpu.py: fills ConvArgs by hand for the layers whose kernel choice the
// comments of csrc/conv_route.cpp document, asks conv_route() and prints one JSON object per line.  No HIP call, nothing
// linked from the library: it is compiled together with csrc/conv_route.cpp alone.  Switches are given as a ConvKnobs value
// built by conv_knobs_from() over a table of this program's own, never through the environment.
#include "conv_route.h"
#include <cstdio>
#include <map>
#include <string>

using namespace evr;

static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
static ConvKnobs knobs(std::map<std::string, std::string> env) { g_env = env; return conv_knobs_from(lookup); }

static float g_ws[4];
static unsigned g_prog[4];
static const float* const PTR = g_ws;

// a k x k stride-1 'same' convolution on PACKED tensors in arithmetic mode x3, ready for the kernels (workspace present)
static ConvArgs conv_same(int n, int h, int w, int c0, int c1, int cout, int epi, int k = 3, int x3 = 3) {
    ConvArgs a = {};
    a.n = n; a.hin = a.hm = a.hout = h; a.win = a.wm = a.wout = w;
    a.c0 = c0; a.c1 = c1; a.in_mode = c1 ? IN_CAT : IN_SINGLE;
    a.stride = 1; a.os = 1; a.cout = cout; a.n_valid = cout; a.cout_total = cout; a.epi = epi;
    a.tp.ntaps = k * k; a.tp.ngroups = 1; a.tp.grp_cols = cout;
    for (int t = 0; t < k * k; ++t) a.tp.set_tap(t, t / k - k / 2, t % k - k / 2, 1);
    a.x3 = x3; a.in_packed = x3 ? 1 : 0; a.acc_scale = 1.f;
    a.ksplit_ws = g_ws;
    if (epi == EPI_LSTM) a.hidden = cout / 4;
    return a;
}
// ConvTranspose2d(k5, s2, p2) as four column groups of a 3x3 convolution on the input grid (model.cpp's plan)
static ConvArgs tconv(int n, int h, int w, int cin, int cout_ch) {
    ConvArgs a = conv_same(n, h, w, cin, 0, 4 * cout_ch, EPI_BIAS_RELU);
    a.os = 2; a.hout = 2 * h; a.wout = 2 * w;
    a.tp.ngroups = 4; a.tp.grp_cols = cout_ch; a.n_valid = cout_ch; a.cout_total = cout_ch;
    for (int t = 0; t < 9; ++t) {
        int groups = 0;
        for (int g = 0; g < 4; ++g) if (!((g >> 1) == 1 && t / 3 == 0) && !((g & 1) == 1 && t % 3 == 0)) groups |= 1 << g;
        a.tp.tap_groups[t] = groups;
    }
    for (int g = 0; g < 4; ++g) { a.tp.grp_ofy[g] = g >> 1; a.tp.grp_ofx[g] = g & 1; }
    return a;
}
// k5 stride-2 encoder convolution with its space-to-depth step program
static ConvArgs enc_k5s2(int n, int hm, int wm, int cin, int cout) {
    ConvArgs a = conv_same(n, hm, wm, cin, 0, cout, EPI_BIAS_RELU, 5);
    a.hin = 2 * hm; a.win = 2 * wm; a.stride = 2;
    a.wgt2 = PTR; a.prog = g_prog; a.prog_steps = 25 * (cin / 32) * 2;
    return a;
}
// one of FireNet's 16-channel layers (residual convolution: one source)
static ConvArgs firenet_res(int n, int h, int w) {
    ConvArgs a = conv_same(n, h, w, 16, 0, 32, EPI_RESIDUAL_RELU);
    a.n_valid = 16; a.cout_total = 16;
    return a;
}

static const char* family_name(int f) {
    static const char* names[] = {"none", "c16_tile", "c16_rows", "band_prog", "band_prog_wide", "band_prog_ksplit", "bandk", "band", "wide", "wide16", "igemm"};
    return names[f];
}
static void show(const char* id, const ConvArgs& a, int kc, int wm, int nb, const ConvKnobs& k) {
    const ConvRoute r = conv_route(a, kc, wm, nb, k);
    printf("{\"id\": \"%s\", \"family\": \"%s\", \"err\": %d, \"kc\": %d, \"wm\": %d, \"nb\": %d, \"x3\": %d, \"phases\": %d, \"wn\": %d, \"kw\": %d, "
           "\"rpb\": %d, \"nsrc\": %d, \"nbuf\": %d, \"lstm\": %d, \"grouped\": %d, \"regstage\": %d, \"alt\": %d, \"tail\": %d, \"halfw\": %d, "
           "\"grid\": %u, \"block\": %u, \"lds\": %zu, \"ks\": %d, \"epi_sum\": %d, \"epi_grid\": %u, \"rseg\": %d, \"nseg\": %d, \"nstrips\": %d}\n",
           id, family_name(r.family), r.err, r.kc, r.wm, r.nb, r.x3, r.phases, r.wn, r.kw, r.rpb, r.nsrc, r.nbuf, (int)r.lstm, (int)r.grouped,
           (int)r.regstage, (int)r.alt, (int)r.tail, (int)r.halfw, r.grid, r.block, r.lds, r.ks, r.epi_sum, r.epi_grid, r.rseg, r.nseg, r.nstrips);
}

int main() {
    const ConvKnobs d = knobs({});
    // E2VID at 346x260 (padded 352x264): encoder grids 176x132, 88x66, 44x33; `seq` sequences
    auto enc0_rec = [](int seq) { return conv_same(seq, 132, 176, 64, 64, 256, EPI_LSTM); };
    auto enc1_rec = [](int seq) { return conv_same(seq, 66, 88, 128, 128, 512, EPI_LSTM); };
    auto enc2_rec = [](int seq) { return conv_same(seq, 33, 44, 256, 256, 1024, EPI_LSTM); };
    auto residual = [](int seq) { return conv_same(seq, 33, 44, 256, 0, 256, EPI_RESIDUAL_RELU); };
    show("enc0.rec.32seq", enc0_rec(32), 32, 4, 4, d);
    show("enc0.rec.64seq", enc0_rec(64), 32, 4, 4, d);
    show("enc0.rec.4seq", enc0_rec(4), 32, 4, 4, d);
    show("enc1.rec.4seq", enc1_rec(4), 32, 4, 4, d);
    show("enc1.rec.8seq", enc1_rec(8), 32, 4, 4, d);
    show("enc2.rec.8seq", enc2_rec(8), 32, 4, 4, d);
    // a ConvLSTM gate launch of 512 input channels with exactly 599 / 600 tiles of 256 x 256
    show("lstm.599", conv_same(1, 599, 256, 256, 256, 256, EPI_LSTM), 32, 4, 4, d);
    show("lstm.600", conv_same(1, 600, 256, 256, 256, 256, EPI_LSTM), 32, 4, 4, d);
    show("residual.64seq", residual(64), 32, 4, 4, d);
    show("residual.128seq", residual(128), 32, 4, 4, d);
    show("dec2.4seq", tconv(4, 132, 176, 64, 32), 32, 4, 4, d);
    show("dec1.8seq", tconv(8, 66, 88, 128, 64), 32, 4, 4, d);
    // a plain 3x3 layer of 256 -> 128 channels with exactly `tiles` 128-pixel tiles
    auto plain = [](int tiles) { return conv_same(1, tiles, 128, 256, 0, 128, EPI_BIAS_RELU); };
    show("band.192", plain(192), 32, 4, 4, d);
    show("band.193", plain(193), 32, 4, 4, d);
    show("band.64", plain(64), 32, 4, 4, d);
    show("band.65", plain(65), 32, 4, 4, d);
    { ConvArgs a = plain(64); a.ksplit_ws = nullptr; show("band.64.no_ws", a, 32, 4, 4, d); }
    // k5 s2 encoders with exactly `tiles` 256-pixel tiles (NB = 2: 32 -> 64 channels) / 128-pixel tiles (NB = 4: 64 -> 128)
    show("enc.nb2.599", enc_k5s2(1, 599, 256, 32, 64), 32, 4, 2, d);
    show("enc.nb2.600", enc_k5s2(1, 600, 256, 32, 64), 32, 4, 2, d);
    show("enc.nb4.599", enc_k5s2(1, 599, 256, 64, 128), 32, 4, 4, d);
    show("enc.nb4.600", enc_k5s2(1, 600, 256, 64, 128), 32, 4, 4, d);
    show("enc.nb4.192", enc_k5s2(1, 192, 128, 64, 128), 32, 4, 4, d);
    show("enc.nb4.193", enc_k5s2(1, 193, 128, 64, 128), 32, 4, 4, d);
    // FireNet residual convolution, 128 x 64 images: 8 (strip, 8-row) items per image -- the row kernel from 1024 items
    show("c16.1016", firenet_res(127, 64, 128), 16, 4, 1, d);
    show("c16.1024", firenet_res(128, 64, 128), 16, 4, 1, d);
    // LPIPS (AlexNet) conv2: 5x5, 64 -> 192 channels, kept off the band form by its plan
    { ConvArgs a = conv_same(8, 15, 20, 64, 0, 192, EPI_BIAS_RELU, 5); show("lpips.conv2.band", a, 32, 4, 2, d); a.no_band5 = 1; show("lpips.conv2", a, 32, 4, 2, d); }

    // ---- switches
    show("ksplit4.band.64", plain(64), 32, 4, 4, knobs({{"EVR_KSPLIT", "4"}}));              // set: the small cap is off -> 4 runs
    show("ksplit16.band.32", plain(32), 32, 4, 4, knobs({{"EVR_KSPLIT", "16"}}));            // 512 / 32 = 16 runs wanted, clamped to 8
    show("ksplit0.band.64", plain(64), 32, 4, 4, knobs({{"EVR_KSPLIT", "0"}}));
    {   // EVR_WIDE_MIN=1 moves all four thresholds: 256 x 256 ConvLSTM, twin ConvLSTM, dec2, plain
        const ConvKnobs k = knobs({{"EVR_WIDE_MIN", "1"}});
        show("wide_min1.enc2.rec.1seq", enc2_rec(1), 32, 4, 4, k);
        show("wide_min1.enc0.rec.1seq", enc0_rec(1), 32, 4, 4, k);
        show("wide_min1.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, k);
        show("wide_min1.dec2.1seq", tconv(1, 132, 176, 64, 32), 32, 4, 4, k);
        show("wide_min1.dec1.1seq", tconv(1, 66, 88, 128, 64), 32, 4, 4, k);
        show("wide_min1.residual.1seq", residual(1), 32, 4, 4, k);
        show("wide_min_plain.residual.1seq", residual(1), 32, 4, 4, knobs({{"EVR_WIDE_MIN_PLAIN", "1"}}));
        show("wide_min_plain.enc0.rec.4seq", enc0_rec(4), 32, 4, 4, knobs({{"EVR_WIDE_MIN_PLAIN", "1"}}));
    }
    show("wide0.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, knobs({{"EVR_WIDE", "0"}}));
    show("wide2.enc2.rec.64seq", enc2_rec(64), 32, 4, 4, knobs({{"EVR_WIDE", "2"}}));
    show("wide3.enc0.rec.32seq", enc0_rec(32), 32, 4, 4, knobs({{"EVR_WIDE", "3"}}));
    show("mfma16_0.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, knobs({{"EVR_MFMA16", "0"}}));
    show("alt0.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, knobs({{"EVR_WIDE16_ALT", "0"}}));
    show("tail0.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, knobs({{"EVR_WIDE16_TAIL", "0"}}));
    show("mx.enc0.rec.64seq", conv_same(64, 132, 176, 64, 64, 256, EPI_LSTM, 3, 2), 32, 4, 4, d);
    show("no_band.enc0.rec.64seq", enc0_rec(64), 32, 4, 4, knobs({{"EVR_NO_BAND", "1"}}));
    show("no_band.enc.nb2.600", enc_k5s2(1, 600, 256, 32, 64), 32, 4, 2, knobs({{"EVR_NO_BAND", "1"}}));
    show("no_band.lpips.conv2.band", conv_same(8, 15, 20, 64, 0, 192, EPI_BIAS_RELU, 5), 32, 4, 2, knobs({{"EVR_NO_BAND", "1"}}));
    show("band5_0.lpips.conv2.band", conv_same(8, 15, 20, 64, 0, 192, EPI_BIAS_RELU, 5), 32, 4, 2, knobs({{"EVR_BAND5", "0"}}));
    show("band5_0.residual.64seq", residual(64), 32, 4, 4, knobs({{"EVR_BAND5", "0"}}));
    show("band_min.residual.1seq", residual(1), 32, 4, 4, knobs({{"EVR_BAND_MIN", "1000"}, {"EVR_BAND5_MIN", "1"}}));
    show("band_min.lpips.conv2.band", conv_same(8, 15, 20, 64, 0, 192, EPI_BIAS_RELU, 5), 32, 4, 2, knobs({{"EVR_BAND_MIN", "1000"}, {"EVR_BAND5_MIN", "1"}}));
    show("rows0.c16.1024", firenet_res(128, 64, 128), 16, 4, 1, knobs({{"EVR_C16_ROWS", "0"}}));
    show("rows2.c16.8", firenet_res(1, 64, 128), 16, 4, 1, knobs({{"EVR_C16_ROWS", "2"}}));
    show("rows_1.c16.1024", firenet_res(128, 64, 128), 16, 4, 1, knobs({{"EVR_C16_ROWS_1", "2,2"}}));
    show("c16_blocks.c16.1016", firenet_res(127, 64, 128), 16, 4, 1, knobs({{"EVR_C16_BLOCKS", "4"}}));
    // the exact-fp32 implicit GEMM (mode 0): ConvLSTM at WM = 4 on register staging, EVR_LSTM_DMA: the DMA loader
    { ConvArgs a = conv_same(1, 33, 44, 256, 256, 1024, EPI_LSTM, 3, 0);
      show("fp32.lstm", a, 32, 4, 4, d); show("fp32.lstm.dma", a, 32, 4, 4, knobs({{"EVR_LSTM_DMA", "1"}}));
      show("fp32.lstm.kc16", a, 16, 4, 4, d); }
    { ConvArgs a = conv_same(1, 33, 44, 16, 0, 32, EPI_BIAS, 3, 0); show("fp32.kc16", a, 16, 2, 1, d); show("fp32.kc16.nb2", a, 16, 2, 2, d); }
    return 0;
}
