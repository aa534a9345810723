// The host side of the VGG-16 trunk: the struct that a metric's handle (lpips_vgg.hip: LPIPS-VGG, dists.hip: DISTS) holds as a member, and
// the loop of its entry point.  The trunk owns everything up to "the features of level l are in buffer s": the folded conv1_1 weights,
// the twelve prepared convolutions, the range counter, the two ping-pong activation buffers and the plans per pair count.  A metric adds
// its state-dict names and input scaling, its pool mode, its head buffers (allocated through `allocs`, so they live and die with the
// trunk's) and its head launches.  Host code only: the kernels are in vgg_backbone.h, conv.hip and the metric's file.
#pragma once
#include <string>
#include <vector>

#include "lpips_host.h"
#include "vgg_backbone.h"

namespace evr {

constexpr size_t ACT_BUDGET_BYTES = (size_t)1 << 30;      // both activation buffers of a handle together (default pass size)
// one buffer, whatever max_pairs asks: conv.hip sizes the buffer descriptor of a tensor in 32-bit bytes and offsets its pixel rows in
// 32-bit float elements (the metrics' own kernels index in 64 bits), and its launcher wants n*hm*wm < 2^31.  2 GiB keeps all three;
// a frame whose single pair does not fit (H*W >= 2^22) is refused by the entry points
constexpr int64_t ACT_BUFFER_MAX_BYTES = (int64_t)1 << 31;

struct VggTrunk {
    using Plan = PlanCache<VGG_NCONV>::Plan;
    std::vector<float> wg, wb, b1, b1in;      // conv1_1 with the input scaling folded in (lpips_host.h fold_scaling_layer)
    float* d_wg = nullptr; float* d_wb = nullptr; float* d_b1 = nullptr; float* d_b1in = nullptr;
    unsigned* d_sat = nullptr;       // range guard of the packed formats (packed.h sat_note): every producer of this handle counts here
    BackboneConv L[VGG_NCONV];
    int mode = 0;                    // arithmetic of the twelve convolutions (lpips_host.h backbone_mode)
    int max_pairs = 0;               // constructor argument: pairs per pass (0: from ACT_BUDGET_BYTES)
    // shape-dependent.  Buffers are sized for `cap` pairs per pass at H x W and only ever grow; what depends on the pair count of
    // a pass (the twelve ConvArgs with their tile choice) lives in the plan cache (lpips_host.h).
    int n = 0, H = 0, W = 0, cap = 0;      // n: pairs of the last call (flops)
    int h[5], w[5];                  // feature map sizes of the five levels
    DeviceAllocs allocs;
    float* act[2] = {nullptr, nullptr};
    PlanCache<VGG_NCONV> plans;
    SplitWorkspace kws;

    // names: conv1_1, then the twelve convolutions of VGG_CIN / VGG_COUT (.weight, .bias); x_c = a_c g + b_c is the metric's input scaling
    int create(const StateDict& sd, const char* const (&names)[VGG_NCONV + 1], const double (&a)[3], const double (&b)[3], int max_pairs_) {
        max_pairs = max_pairs_;
        mode = backbone_mode();
        int rc;
        const evr_tensor *w1, *bias1;
        if ((rc = sd.get(std::string(names[0]) + ".weight", 64 * 3 * 9, &w1))) return rc;
        if ((rc = sd.get(std::string(names[0]) + ".bias", 64, &bias1))) return rc;
        fold_scaling_layer(w1->data_host, bias1->data_host, 64, 9, a, b, wg, wb, b1, b1in);
        if ((rc = upload(wg, &d_wg)) || (rc = upload(wb, &d_wb)) || (rc = upload(b1, &d_b1)) || (rc = upload(b1in, &d_b1in))) return rc;
        for (int l = 0; l < VGG_NCONV; ++l)
            if ((rc = prepare_backbone_conv(sd, names[l + 1], VGG_CIN[l], VGG_COUT[l], 3, mode, &L[l]))) return rc;
        EVR_HIP(hipMalloc((void**)&d_sat, 64));
        EVR_HIP(hipMemset(d_sat, 0, 64));
        return EVR_OK;
    }

    // pairs per pass at H x W
    int pass_pairs(int H_, int W_) const {
        const int64_t per_pair = (int64_t)2 * H_ * W_ * 64 * 4;      // one buffer, one pair
        int64_t p = max_pairs > 0 ? max_pairs : (int64_t)(ACT_BUDGET_BYTES / 2) / per_pair;
        if (p * per_pair >= ACT_BUFFER_MAX_BYTES) p = (ACT_BUFFER_MAX_BYTES - 1) / per_pair;      // (>= 1: the entry points refuse larger frames)
        return p < 1 ? 1 : (int)p;
    }

    // (re)allocate the activation buffers for `cap` pairs per pass of H x W, a pool halving a side downwards or (ceil_pool) upwards: the
    // only place that synchronises.  The metric allocates its head buffers through `allocs` afterwards.
    int buffers(int cap_, int H_, int W_, bool ceil_pool, hipStream_t stream) {
        EVR_HIP(hipStreamSynchronize(stream));
        release();
        cap = cap_; H = H_; W = W_;
        h[0] = H; w[0] = W;
        for (int l = 1; l < 5; ++l) { h[l] = (h[l - 1] + ceil_pool) / 2; w[l] = (w[l - 1] + ceil_pool) / 2; }
        int rc;
        // the largest layer: relu1_1 / relu1_2 (a pooled map has at most ((H+1)/2)((W+1)/2) <= HW/2 pixels of twice the channels from 3 x 3 on)
        const size_t numel = (size_t)2 * cap * H * W * 64;
        for (int i = 0; i < 2; ++i) if ((rc = allocs.alloc(&act[i], numel))) return rc;
        return allocs.alloc(&plans.d_args, (size_t)plans.NPLANS * VGG_NCONV);
    }
    // frees the buffers, the metric's among them: its release() clears its own pointers beside this
    void release() {
        allocs.release();
        cap = 0; plans.clear(); kws = SplitWorkspace(); act[0] = act[1] = nullptr;
    }

    // the plan of n pairs inside the current buffers (PlanCache::get fills a slot with this)
    void fill_plan(Plan& pl, int n_) {
        for (int i = 0; i < VGG_NCONV; ++i) {
            ConvArgs& a = pl.args[i];
            const int lv = VGG_LEVEL[i], src = vgg_conv_src(i);
            fill_backbone_conv(a, L[i], act[src], act[src ^ 1], 2 * n_, h[lv], w[lv]);
            a.sat = d_sat;
            pick_conv_tile(a, 32, &pl.wm[i], &pl.nb[i]);
        }
        attach_split_workspace(kws, allocs, pl.args, VGG_NCONV, 0);
    }

    // ---- one pass of np pairs: begin_pass, conv1_1, then level_convs for levels 0 .. 4 with the metric's pool between them ----------
    int begin_pass(int np, hipStream_t stream, Plan** P) {
        return plans.get(np, stream, [this](Plan& pl, int n_) { fill_plan(pl, n_); }, P);
    }
    int fmt() const { return packed_fmt(mode); }      // the activation format of both buffers
    // img / ref [np,H,W] -> relu1_1 of the 2 np frames in buffer 0
    int conv1_1(const float* img, const float* ref, int np, int clip, hipStream_t stream) {
        Conv11Args c1{};
        c1.img = img; c1.ref = ref; c1.n = np; c1.H = H; c1.W = W; c1.clip = clip;
        c1.wg = d_wg; c1.wb = d_wb; c1.bias = d_b1; c1.bias_in = d_b1in; c1.out = act[0]; c1.sat = d_sat;
        return launch_conv1_1_fmt(fmt(), c1, stream);
    }
    // the convolutions of `level`, whose input (conv1_1's output, or the pool of the level before) the caller has put where
    // vgg_conv_src says.  *feat: the buffer the level's features now sit in; its pool goes to the other one, *feat ^ 1
    int level_convs(const Plan* P, int level, hipStream_t stream, int* feat) {
        ConvArgs* const d_args = plans.device_args(P);
        int rc;
        for (int i = 0; i < VGG_NCONV; ++i) {
            if (VGG_LEVEL[i] != level) continue;
            if ((rc = launch_conv_igemm(P->args[i], d_args + i, 32, P->wm[i], P->nb[i], stream))) return rc;
            *feat = vgg_conv_src(i) ^ 1;
        }
        return EVR_OK;
    }

    // algorithmic operations of the last call: 2 per multiply-add of the thirteen convolutions, conv1_1 in the folded one-channel form it
    // runs in (304,704 multiply-adds per input pixel at sides that are multiples of 16)
    double flops() const {
        if (n == 0) return 0.0;
        double f = 2.0 * (2.0 * n) * H * W * 64 * 9;
        for (int l = 0; l < VGG_NCONV; ++l) f += 2.0 * (2.0 * n) * h[VGG_LEVEL[l]] * w[VGG_LEVEL[l]] * VGG_CIN[l] * VGG_COUT[l] * 9;
        return f;
    }
    // the range-guard counter (output runs beyond the packed format's exact range, packed.h sat_note) since the last read; cleared.
    // Waits for the stream.
    int saturation(int64_t* count, hipStream_t stream) {
        unsigned v = 0;
        EVR_HIP(hipMemcpyAsync(&v, d_sat, sizeof(v), hipMemcpyDeviceToHost, stream));
        EVR_HIP(hipMemsetAsync(d_sat, 0, sizeof(v), stream));
        EVR_HIP(hipStreamSynchronize(stream));
        *count = (int64_t)v;
        return EVR_OK;
    }

    ~VggTrunk() {
        release();
        for (void* p : {(void*)d_wg, (void*)d_wb, (void*)d_b1, (void*)d_b1in, (void*)d_sat}) if (p) (void)hipFree(p);
        for (auto& l : L) free_backbone_conv(l);
    }
};

// The body of a metric's forward entry point after its checks.  m: the handle, with the members `trunk`, `release()` and
// `buffers(cap, H, W, stream)` -- trunk.buffers in the metric's pool mode, then its head buffers.  The buffers are reallocated when the
// frame size changes or a pass needs more pairs than they hold; pass(o, np) scores pairs o .. o + np, both frames of a pair always in
// the same pass.
template <typename M, typename Pass>
int vgg_forward(M* m, int n, int H, int W, hipStream_t stream, Pass pass) {
    VggTrunk& t = m->trunk;
    int rc;
    const int P = t.pass_pairs(H, W), need = n < P ? n : P;
    if (t.H != H || t.W != W || need > t.cap) if ((rc = m->buffers(need, H, W, stream))) { m->release(); t.H = t.W = 0; return rc; }
    t.n = n;
    for (int o = 0; o < n; o += P) if ((rc = pass(o, n - o < P ? n - o : P))) return rc;
    return EVR_OK;
}

}  // namespace evr
