// Stand-alone host program of tests/test_knobs_cpu.py: fills the LibKnobs table (csrc/knobs.h) for one environment after another and
// prints one JSON object per line.  No HIP call, nothing linked from the library: it is compiled together with csrc/knobs.cpp alone.
// An environment is a map of this program's own, never the process's: every switch with each of "0", "1", the empty string and a
// non-number, then the values that mean something else for one switch (negative numbers, the arithmetic names, two switches together).
#include "knobs.h"
#include <cstdio>
#include <map>
#include <string>
#include <vector>

using namespace evr;

typedef std::map<std::string, std::string> Env;
static Env g_env;
static const char* lookup(const char* name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

// the row's id is the environment itself: NAME=value pairs in the map's order, blank-separated ("empty": none)
static void row(const Env& env) {
    g_env = env;
    const LibKnobs k = lib_knobs_from(lookup);
    std::string id;
    for (const auto& kv : env) id += (id.empty() ? "" : " ") + kv.first + "=" + kv.second;
    printf("{\"id\": \"%s\", \"arith\": %d, \"group_store\": %d, \"tconv_inter\": %d, \"firenet_h3\": %d, \"firenet_pad32\": %d, \"wino\": %d, "
           "\"wino_tconv\": %d, \"wino_s2d\": %d, \"no_pred_dot\": %d, \"wino_blocks\": %d, \"wino_fastact\": %d, \"wino_order\": %d, "
           "\"head_wlds\": %d, \"head_blocks\": %d, \"lpips_band5_kb\": %d, \"lpips_conv1_valu\": %d, \"lpips_score_split\": %d, "
           "\"pct_pair\": %d, \"pct_fast\": %d, \"vox_acc_kb_set\": %d, \"vox_acc_kb\": %d, \"vox_split\": %d, \"vox_chunks\": %d, "
           "\"attn_valu\": %d, \"png_per_dir\": %d, \"ablate\": %d, \"ablate_all\": %d, \"wino_var\": %d, \"vox_scanprobe\": %d}\n",
           id.empty() ? "empty" : id.c_str(), k.arith, k.group_store, (int)k.tconv_inter, (int)k.firenet_h3, (int)k.firenet_pad32, (int)k.wino,
           (int)k.wino_tconv, (int)k.wino_s2d, (int)k.no_pred_dot, k.wino_blocks, (int)k.wino_fastact, k.wino_order,
           k.head_wlds, k.head_blocks, k.lpips_band5_kb, (int)k.lpips_conv1_valu, k.lpips_score_split,
           k.pct_pair, k.pct_fast, (int)k.vox_acc_kb_set, k.vox_acc_kb, k.vox_split, k.vox_chunks,
           (int)k.attn_valu, k.png_per_dir, k.ablate, (int)k.ablate_all, k.wino_var, k.vox_scanprobe);
}

int main() {
    row({});
    const char* names[] = {"EVR_FP32", "EVR_ARITH", "EVR_GROUP_STORE", "EVR_TCONV_INTER", "EVR_FIRENET_H3", "EVR_FIRENET_PAD32", "EVR_WINO",
                           "EVR_WINO_TCONV", "EVR_WINO_S2D", "EVR_NO_PRED_DOT", "EVR_WINO_BLOCKS", "EVR_WINO_FASTACT", "EVR_WINO_ORDER",
                           "EVR_HEAD_WLDS", "EVR_HEAD_BLOCKS", "EVR_LPIPS_BAND5", "EVR_LPIPS_CONV1_VALU", "EVR_LPIPS_SCORE_SPLIT",
                           "EVR_PCT_PAIR", "EVR_PCT_FAST", "EVR_VOX_ACC_KB", "EVR_VOX_SPLIT", "EVR_VOX_CHUNKS", "EVR_ATTN_VALU",
                           "EVREAL_PNG_PER_DIR", "EVR_ABLATE", "EVR_ABLATE_ALL", "EVR_WINO_VAR", "EVR_VOX_SCANPROBE"};
    for (const char* n : names)
        for (const char* v : {"0", "1", "", "abc"}) row({{n, v}});
    const std::vector<Env> more = {
        // the arithmetic rule
        {{"EVR_ARITH", "h3"}}, {{"EVR_ARITH", "mx6"}}, {{"EVR_ARITH", "mx"}}, {{"EVR_ARITH", "fp32"}},
        {{"EVR_FP32", "1"}, {"EVR_ARITH", "mx"}}, {{"EVR_FP32", "0"}, {"EVR_ARITH", "mx6"}},
        // numbers: negative, larger, with a tail
        {{"EVR_WINO_BLOCKS", "-3"}}, {{"EVR_WINO_BLOCKS", "128"}}, {{"EVR_WINO_BLOCKS", "12abc"}},
        {{"EVR_HEAD_BLOCKS", "-2"}}, {{"EVR_HEAD_BLOCKS", "1024"}}, {{"EVR_HEAD_WLDS", "1"}, {"EVR_HEAD_BLOCKS", "300"}}, {{"EVR_HEAD_WLDS", "1"}, {"EVR_HEAD_BLOCKS", "0"}},
        {{"EVR_LPIPS_BAND5", "-1"}}, {{"EVR_LPIPS_BAND5", "16"}}, {{"EVR_LPIPS_SCORE_SPLIT", "2"}},
        {{"EVR_GROUP_STORE", "2"}}, {{"EVR_WINO_ORDER", "-1"}}, {{"EVR_PCT_PAIR", "2"}}, {{"EVR_PCT_FAST", "-1"}},
        {{"EVR_FIRENET_PAD32", "2"}}, {{"EVR_ATTN_VALU", "-1"}}, {{"EVR_WINO", "-1"}}, {{"EVR_TCONV_INTER", " 0"}},
        {{"EVR_VOX_ACC_KB", "-1"}}, {{"EVR_VOX_ACC_KB", "64"}}, {{"EVR_VOX_ACC_KB", "500"}}, {{"EVR_VOX_SPLIT", "4"}}, {{"EVR_VOX_SPLIT", "-1"}},
        {{"EVR_VOX_CHUNKS", "4"}}, {{"EVR_VOX_CHUNKS", "-1"}},
        {{"EVREAL_PNG_PER_DIR", "8"}}, {{"EVREAL_PNG_PER_DIR", "-1"}},
        // the timing experiments
        {{"EVR_ABLATE", "5"}}, {{"EVR_ABLATE", "-1"}}, {{"EVR_ABLATE", "3"}, {"EVR_ABLATE_ALL", "1"}}, {{"EVR_ABLATE_ALL", "0"}, {"EVR_ABLATE", "16"}},
        {{"EVR_WINO_VAR", "2"}}, {{"EVR_WINO_VAR", "4"}}, {{"EVR_VOX_SCANPROBE", "2"}},
    };
    for (const Env& e : more) row(e);
    return 0;
}
