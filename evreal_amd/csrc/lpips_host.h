// Host set-up shared by the backbone metrics (lpips.hip: AlexNet, lpips_vgg.hip and dists.hip: VGG-16): the state-dict lookup, the fold of
// the input scaling into a one-channel first convolution, a backbone convolution prepared for the kernels of conv.hip and
// its ConvArgs, the per-pair-count plan cache, the split-K workspace and the device allocations of a handle.  Host code only;
// every kernel stays in its backbone's file.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "conv.h"

namespace evr {

// the tensors of a state dict by name; `label` ("LPIPS", "LPIPS-VGG") names the metric in the messages
struct StateDict {
    const char* label;
    std::map<std::string, const evr_tensor*> sd;
    StateDict(const char* label_, const evr_tensor* tensors, int n_tensors) : label(label_) {
        for (int i = 0; i < n_tensors; ++i) if (tensors[i].name) sd[tensors[i].name] = &tensors[i];
    }
    int get(const std::string& k, int64_t numel, const evr_tensor** t) const {
        auto it = sd.find(k);
        if (it == sd.end()) { set_error("%s state_dict is missing '%s'", label, k.c_str()); return EVR_ERR_MISSING_TENSOR; }
        int64_t ne = 1; for (int d = 0; d < it->second->ndim; ++d) ne *= it->second->shape[d];
        if (ne != numel) { set_error("%s tensor '%s' has %lld elements, expected %lld", label, k.c_str(), (long long)ne, (long long)numel); return EVR_ERR_INVALID; }
        *t = it->second; return EVR_OK;
    }
};

// device allocations that live as long as a handle's buffers (released together when the shape changes)
struct DeviceAllocs {
    std::vector<void*> ptrs;
    template <typename T>
    int alloc(T** p, size_t count) {
        EVR_HIP(hipMalloc((void**)p, count * sizeof(T) + 256));
        ptrs.push_back((void*)*p);
        return EVR_OK;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// An input scaling folded into a first convolution (w [cout][3][taps], OIHW) that reads the gray frame: the three input channels
// are x_c = a_c * g + b_c, so wg = sum_c w a_c and wb = sum_c w b_c (both [taps][cout], fp64 sums rounded once) make it a
// one-channel convolution plus the wb term where the window is inside the image; b1in = bias + sum_t wb[t] is the bias of a window
// that lies wholly inside.
inline void fold_scaling_layer(const float* w, const float* bias, int cout, int taps, const double (&a)[3], const double (&b)[3],
                               std::vector<float>& wg, std::vector<float>& wb, std::vector<float>& b1, std::vector<float>& b1in) {
    wg.assign((size_t)taps * cout, 0.f); wb.assign((size_t)taps * cout, 0.f);
    b1.assign(bias, bias + cout); b1in.assign(cout, 0.f);
    for (int co = 0; co < cout; ++co) {
        double bsum = 0.0;
        for (int t = 0; t < taps; ++t) {
            double g = 0.0, bb = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double wv = w[((size_t)co * 3 + c) * taps + t];
                g += wv * a[c]; bb += wv * b[c];
            }
            wg[(size_t)t * cout + co] = (float)g; wb[(size_t)t * cout + co] = (float)bb;
            bsum += bb;
        }
        b1in[co] = (float)((double)b1[co] + bsum);
    }
}
// The scaling layer of LPIPS, x_c = ((2g-1) - shift_c)/scale_c, as (a_c, b_c)
inline void lpips_scaling(double (&a)[3], double (&b)[3]) {
    const double shift[3] = {-.030, -.088, -.188}, scale[3] = {.458, .448, .450};
    for (int c = 0; c < 3; ++c) { a[c] = 2.0 / scale[c]; b[c] = (-1.0 - shift[c]) / scale[c]; }
}
inline void fold_scaling_layer(const float* w, const float* bias, int cout, int taps, std::vector<float>& wg, std::vector<float>& wb,
                               std::vector<float>& b1, std::vector<float>& b1in) {
    double a[3], b[3];
    lpips_scaling(a, b);
    fold_scaling_layer(w, bias, cout, taps, a, b, wg, wb, b1, b1in);
}

// arithmetic of the backbone convolutions: the networks' mode, except that P6 tensors (mode 4) have no 4-channel writer -- the
// pools, the first convolution's epilogue -- so LPIPS keeps the fp8 form there
inline int backbone_mode() { const int m = arith_mode(); return m == 4 ? 2 : m; }

// one k x k stride-1 same-padding bias + ReLU convolution of a backbone, on the device in the form conv.hip wants
struct BackboneConv {
    int cin = 0, cout = 0, k = 0;
    int x3 = 0, mx_e = 0;            // arithmetic mode, weight exponent (pack_weights_for)
    float* d_w = nullptr; float* d_b = nullptr;
    float* d_wino = nullptr;         // exact-fp32 mode, 3x3 layers: Winograd-domain weights (wino.hip), or null
};

// `name`.weight [cout][cin][k][k] and `name`.bias of the state dict -> the layer: weights transposed to [cout][tap][cin] and packed
// for `mode`, the bias in the mode's product scale (conv.h prescale_bias).  The packed host copy (9 MB for a 512 x 512 layer) is
// not kept.
inline int prepare_backbone_conv(const StateDict& sd, const std::string& name, int cin, int cout, int k, int mode, BackboneConv* L) {
    const int taps = k * k;
    const evr_tensor *w, *b;
    int rc;
    if ((rc = sd.get(name + ".weight", (int64_t)cout * cin * taps, &w))) return rc;
    if ((rc = sd.get(name + ".bias", cout, &b))) return rc;
    L->cin = cin; L->cout = cout; L->k = k; L->x3 = mode;
    std::vector<float> wt((size_t)cout * taps * cin, 0.f), bias(b->data_host, b->data_host + cout);
    for (int co = 0; co < cout; ++co) for (int ci = 0; ci < cin; ++ci) for (int t = 0; t < taps; ++t)
        wt[((size_t)co * taps + t) * cin + ci] = w->data_host[((size_t)co * cin + ci) * taps + t];
    // exact-fp32 mode: 3x3 layers also get their Winograd-domain weights (as model.cpp finish_conv; EVR_WINO=0: never)
    if (mode == 0 && k == 3 && wino_enabled() && cin % 16 == 0 && cout % 64 == 0) {
        std::vector<float> u;
        wino_pack_weights(wt, cout, cin, 0, u);
        if ((rc = upload(u, &L->d_wino))) return rc;
    }
    if (mode) L->mx_e = pack_weights_for(mode, wt);
    prescale_bias(mode, L->mx_e, bias);
    if ((rc = upload(wt, &L->d_w))) return rc;
    return upload(bias, &L->d_b);
}
inline void free_backbone_conv(BackboneConv& L) {
    if (L.d_w) (void)hipFree(L.d_w); if (L.d_b) (void)hipFree(L.d_b); if (L.d_wino) (void)hipFree(L.d_wino);
    L.d_w = L.d_b = L.d_wino = nullptr;
}

// ConvArgs of layer L on the NHWC tensor `in` [n2, h, w, cin] -> `out` [n2, h, w, cout]; both are PACKED (H2 in mode 3) in the split
// modes, PLAIN in the fp32 mode.  The caller adds what is its own, then picks the tile (pick_conv_tile).
inline void fill_backbone_conv(ConvArgs& a, const BackboneConv& L, const float* in, float* out, int n2, int h, int w) {
    memset(&a, 0, sizeof(a));
    a.in0 = in; a.c0 = L.cin; a.in_mode = IN_SINGLE; a.n = n2; a.hin = h; a.win = w;
    a.hm = h; a.wm = w; a.stride = 1; a.os = 1; a.hout = h; a.wout = w;
    const int pad = L.k / 2;
    a.tp.ntaps = L.k * L.k; a.tp.ngroups = 1; a.tp.grp_cols = L.cout;
    for (int ky = 0; ky < L.k; ++ky) for (int kx = 0; kx < L.k; ++kx) a.tp.set_tap(ky * L.k + kx, ky - pad, kx - pad, 1);
    a.wgt = L.d_w; a.bias = L.d_b; a.cout = L.cout; a.n_valid = L.cout; a.out = out; a.cout_total = L.cout;
    a.epi = EPI_BIAS_RELU;
    a.wgt_wino = L.d_wino; set_wino_grid(a);
    a.in_packed = a.out_packed = L.x3 ? 1 : 0;
    set_mode_fields(a, L.x3, L.mx_e);
}

// Split-K partial sums at small batches (conv.h KSPLIT_WS_BYTES): a handle's own -- it runs on the evaluation stream beside a
// model's launches.  Allocated on the first plan with a convolution that can split -- a split arithmetic and <= 192 tiles of 128
// pixels -- and a failed allocation degrades to "never split" instead of failing the plan.
struct SplitWorkspace { float* p = nullptr; bool tried = false; };
// sets ksplit_ws of args[0 .. count): the workspace if one of args[first .. count) can split, else null
inline void attach_split_workspace(SplitWorkspace& ws, DeviceAllocs& allocs, ConvArgs* args, int count, int first) {
    bool may_split = false;
    for (int i = first; i < count; ++i) if (args[i].x3 && (int64_t)args[i].n * args[i].hm * args[i].wm <= 192LL * 128) may_split = true;
    if (may_split && !ws.p && !ws.tried) {
        ws.tried = true;
        if (hipMalloc((void**)&ws.p, KSPLIT_WS_BYTES) != hipSuccess) { (void)hipGetLastError(); ws.p = nullptr; }
        else allocs.ptrs.push_back((void*)ws.p);
    }
    for (int i = 0; i < count; ++i) args[i].ksplit_ws = may_split ? ws.p : nullptr;
}

// What depends on the pair count n of a launch set -- the NC ConvArgs with their tile choice -- lives in a small cache of plans
// inside the handle's current buffers.  Round 6: the drop-in's chunks change n at every sequence boundary (a short last chunk, then
// a full one), and the one-plan form answered each change with a stream synchronise + hipFree + hipMalloc of everything -- 16
// device-wide stalls in an eight-sequence run.
template <int NC>
struct PlanCache {
    struct Plan { int n = 0; unsigned stamp = 0; ConvArgs args[NC]; int wm[NC], nb[NC]; };
    static constexpr int NPLANS = 8;
    Plan plans[NPLANS]; unsigned clock = 0;
    ConvArgs* d_args = nullptr;      // [NPLANS][NC], allocated with the buffers
    void clear() { d_args = nullptr; for (auto& pl : plans) pl.n = 0; }
    ConvArgs* device_args(const Plan* pl) const { return d_args + NC * (pl - plans); }
    // the plan of n pairs: cached, or filled by fill(plan, n) into the first empty, else the least recently used slot (its ConvArgs
    // go to the device in stream order, behind whatever launch still reads the slot's previous contents)
    template <typename Fill>
    int get(int n, hipStream_t stream, Fill fill, Plan** out) {
        Plan* pl = nullptr;
        for (auto& c : plans) if (c.n == n) pl = &c;
        if (pl) { pl->stamp = ++clock; *out = pl; return EVR_OK; }
        for (auto& c : plans) {
            if (c.n == 0) { pl = &c; break; }
            if (!pl || c.stamp < pl->stamp) pl = &c;
        }
        pl->n = 0;
        fill(*pl, n);
        EVR_HIP(hipMemcpyAsync(device_args(pl), pl->args, NC * sizeof(ConvArgs), hipMemcpyHostToDevice, stream));
        pl->n = n; pl->stamp = ++clock; *out = pl;
        return EVR_OK;
    }
};

}  // namespace evr
