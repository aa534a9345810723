// The library's run-time switches outside the conv dispatch (host only, no HIP call): how an environment value is parsed, and the
// one table of them, read once per process.  The conv dispatch's own table, ConvKnobs, is in conv_route.h and parses with the same
// helpers.  Nothing else under csrc/ reads the environment.
#pragma once
#include <cstdlib>
#include <cstring>

namespace evr {

// an environment: getenv or a stand-in (the CPU tests pass a map)
using KnobGet = const char* (*)(const char*);

// ---- the parse idioms (inline: conv_route.cpp, which the CPU tests compile on its own, parses ConvKnobs with them)
// atoi of the value, `dflt` when unset (empty or not a number: 0)
inline int knob_num(KnobGet get, const char* name, int dflt) { const char* e = get(name); return e ? atoi(e) : dflt; }
// <first>,<second>: atoi of what follows the comma, `dflt` without one (either part may be missing)
inline int knob_second(KnobGet get, const char* name, int dflt) { const char* e = get(name); const char* c = e ? strchr(e, ',') : nullptr; return c ? atoi(c + 1) : dflt; }
// set, any value (empty and 0 included)
inline bool knob_set(KnobGet get, const char* name) { return get(name) != nullptr; }
// on unless set to something whose atoi is 0
inline bool knob_on(KnobGet get, const char* name) { return knob_num(get, name, 1) != 0; }

// Every switch the library reads outside the conv dispatch (README "Run-time switches" lists them in this order).  Fields hold the
// values in force: a default that depends on another switch is resolved where the table is filled (lib_knobs_from).
struct LibKnobs {
    // ---- arithmetic (conv.h arith_mode / use_group_store)
    int arith = 3;                  // EVR_FP32 (set, any value -- 0 too): 0 exact fp32.  Else EVR_ARITH: h3 -> 3 (also unset, empty, anything unknown), mx6 -> 4, mx -> 2, fp32 -> 0
    int group_store = 1;            // EVR_GROUP_STORE=0: PACKED tensors written and read in 4-channel pieces, not whole groups (A/B; mx6 then narrows to mx)
    // ---- model build (model.cpp)
    bool tconv_inter = true;        // EVR_TCONV_INTER=0: phase-major transposed decoders (default: the four phases interleaved per 128-column tile)
    bool firenet_h3 = true;         // EVR_FIRENET_H3=0: FireNet's 16-channel layers on the exact-fp32 path in the split modes too
    bool firenet_pad32 = false;     // EVR_FIRENET_PAD32=1: FireNet's 16 channels padded to 32, on the split kernels
    bool wino = true;               // EVR_WINO=0: no Winograd F(2x2, 3x3) in the exact-fp32 mode -- the direct implicit GEMM
    bool wino_tconv = true;         // EVR_WINO_TCONV=0: only the transposed decoders back on the direct form
    bool wino_s2d = true;           // EVR_WINO_S2D=0: only the k5 stride-2 encoders back on the direct form
    bool no_pred_dot = false;       // EVR_NO_PRED_DOT (set, any value): the last decoder loads the prediction layer's skip channels itself
    // ---- Winograd launch (wino.hip, set_wino_grid)
    int wino_blocks = 256;          // EVR_WINO_BLOCKS=<n>: persistent blocks (default, and for n <= 0: 256, one per CU)
    bool wino_fastact = true;       // EVR_WINO_FASTACT=0: libm-grade gate activations in the ConvLSTM form
    int wino_order = 1;             // EVR_WINO_ORDER=0: column-block-fastest work order (default 1)
    // ---- head convolution (conv_misc.hip)
    int head_wlds = 0;              // EVR_HEAD_WLDS=1: the matrix-core head kernel with its weights in LDS, three work-groups per CU (A/B; default 0: in registers)
    int head_blocks = 512;          // EVR_HEAD_BLOCKS=<n>: work-groups of the persistent head kernel (default, and for n <= 0: EVR_HEAD_WLDS ? 768 : 512)
    // ---- LPIPS (lpips.hip)
    int lpips_band5_kb = 8;         // EVR_LPIPS_BAND5=<KB>: conv2 on the band kernel with that much LDS padding (default 8); negative: on the implicit GEMM
    bool lpips_conv1_valu = false;  // EVR_LPIPS_CONV1_VALU (set, any value): the direct VALU conv1 kernel in the split modes too (A/B)
    int lpips_score_split = 1;      // EVR_LPIPS_SCORE_SPLIT: 0 the layer scores in one launch, 1 relu3-5 together (default), 2 one launch per layer
    // ---- pre / post-processing (prepost.hip)
    int pct_pair = 1;               // EVR_PCT_PAIR=0: the four-pass percentile select with one work-group per order statistic, not one per percentile
    int pct_fast = 1;               // EVR_PCT_FAST=0: the four-pass percentile select, not the one-pass sampled-bracket form
    // ---- tensorizer (voxelize.hip)
    bool vox_acc_kb_set = false;    // EVR_VOX_ACC_KB=<KB>: LDS for the cells of a range (tuning).  Unset: voxelize.hip's ACC_KB_DEFAULT; it clamps
    int vox_acc_kb = 0;             //   the value to [8, 128] either way
    int vox_split = 0;              // EVR_VOX_SPLIT=<n>: split work-groups per window (tuning; default, and for n <= 0: by the average window, 1..32)
    int vox_chunks = 0;             // EVR_VOX_CHUNKS=<n>: chunks of windows on two streams (default, and for n <= 0: 2 from 2048 windows on, else 1)
    // ---- ET-Net (etnet.hip)
    bool attn_valu = false;         // EVR_ATTN_VALU=1: the VALU attention kernel, not the matrix-core one (A/B)
    // ---- host codec (hostcodec.cpp)
    int png_per_dir = 0;            // EVREAL_PNG_PER_DIR=<n>, n >= 1: PNG writers at work in one directory at a time (default, and for n < 1: the pool's own 4)
    // ---- timing experiments whose RESULTS ARE GARBAGE by design: never set for a run whose output is used
    int ablate = 0;                 // EVR_ABLATE=<mask>: parts of the conv kernels skipped (ConvArgs::debug_ablate: bit 0 barriers, 1 DMA, 2 epilogue math, 4 operand loads); ConvLSTM layers only
    bool ablate_all = false;        // EVR_ABLATE_ALL (set, any value): ... every planned conv
    int wino_var = 0;               // EVR_WINO_VAR=2|4: the ConvLSTM Winograd kernel without its side work | with it on cache-hot addresses (wino.hip VAR); any other value: the kernel as it is
    int vox_scanprobe = 0;          // EVR_VOX_SCANPROBE=1|2: the range kernel scanning the raw events itself (voxelize.hip SCAN; raw-event calls only)
};
// the table for a given environment, and the process's own, filled whole on first use
LibKnobs lib_knobs_from(KnobGet get);
const LibKnobs& lib_knobs();

}  // namespace evr
