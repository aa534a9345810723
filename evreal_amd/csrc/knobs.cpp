// The LibKnobs table (knobs.h): how it is filled from an environment, and the process's own.  The only getenv of the library besides conv_knobs().
#include "knobs.h"

namespace evr {

namespace {

// conv.h arith_mode(): 3 h3 (the default), 4 mx6, 2 mx, 0 exact fp32
int arith_from(KnobGet get) {
    if (knob_set(get, "EVR_FP32")) return 0;
    const char* e = get("EVR_ARITH");
    if (!e || !*e || !strcmp(e, "h3")) return 3;
    if (!strcmp(e, "mx6")) return 4;
    if (!strcmp(e, "mx")) return 2;
    if (!strcmp(e, "fp32")) return 0;
    return 3;
}

}  // namespace

LibKnobs lib_knobs_from(KnobGet get) {
    LibKnobs k;
    k.arith = arith_from(get);
    k.group_store = knob_num(get, "EVR_GROUP_STORE", 1);
    k.tconv_inter = knob_on(get, "EVR_TCONV_INTER");
    k.firenet_h3 = knob_on(get, "EVR_FIRENET_H3");
    k.firenet_pad32 = knob_num(get, "EVR_FIRENET_PAD32", 0) != 0;
    k.wino = knob_on(get, "EVR_WINO");
    k.wino_tconv = knob_on(get, "EVR_WINO_TCONV");
    k.wino_s2d = knob_on(get, "EVR_WINO_S2D");
    k.no_pred_dot = knob_set(get, "EVR_NO_PRED_DOT");
    k.wino_blocks = knob_num(get, "EVR_WINO_BLOCKS", 0) > 0 ? knob_num(get, "EVR_WINO_BLOCKS", 0) : 256;
    k.wino_fastact = knob_on(get, "EVR_WINO_FASTACT");
    k.wino_order = knob_num(get, "EVR_WINO_ORDER", 1);
    k.head_wlds = knob_num(get, "EVR_HEAD_WLDS", 0);
    k.head_blocks = knob_num(get, "EVR_HEAD_BLOCKS", 0) > 0 ? knob_num(get, "EVR_HEAD_BLOCKS", 0) : (k.head_wlds ? 768 : 512);
    k.lpips_band5_kb = knob_num(get, "EVR_LPIPS_BAND5", 8);
    k.lpips_conv1_valu = knob_set(get, "EVR_LPIPS_CONV1_VALU");
    k.lpips_score_split = knob_num(get, "EVR_LPIPS_SCORE_SPLIT", 1);
    k.pct_pair = knob_num(get, "EVR_PCT_PAIR", 1);
    k.pct_fast = knob_num(get, "EVR_PCT_FAST", 1);
    k.vox_acc_kb_set = knob_set(get, "EVR_VOX_ACC_KB");
    k.vox_acc_kb = knob_num(get, "EVR_VOX_ACC_KB", 0);
    k.vox_split = knob_num(get, "EVR_VOX_SPLIT", 0);
    k.vox_chunks = knob_num(get, "EVR_VOX_CHUNKS", 0);
    k.attn_valu = knob_num(get, "EVR_ATTN_VALU", 0) != 0;
    k.png_per_dir = knob_num(get, "EVREAL_PNG_PER_DIR", 0);
    k.ablate = knob_num(get, "EVR_ABLATE", 0);
    k.ablate_all = knob_set(get, "EVR_ABLATE_ALL");
    k.wino_var = knob_num(get, "EVR_WINO_VAR", 0);
    k.vox_scanprobe = knob_num(get, "EVR_VOX_SCANPROBE", 0);
    return k;
}
const LibKnobs& lib_knobs() {
    static const LibKnobs k = lib_knobs_from([](const char* name) -> const char* { return getenv(name); });
    return k;
}

}  // namespace evr
