// Probe (not part of the product): on which SIMD does each of the eight waves of a 512-thread block run?  The skewed loop of
// conv3x3_wide16_kernel<2, true> (csrc/conv.hip, alt16) wants the two waves of a SIMD in different halves of the block, and takes
// waves w and w + 4 for a pair.  Blocks with the kernel's shape (512 threads, 133,248 B of LDS: one block per CU), two rounds of them;
// lane 0 of every wave stores its hardware-id register (HW_ID: wave slot bits 3:0, SIMD 5:4, CU 11:8, SE 15:13).  Prints how many
// blocks have simd(w) == simd(w + 4) for w = 0..3 with four different SIMDs, and every other pattern seen.
//   hipcc --offload-arch=gfx950 -O3 tools/wave_simd_probe.hip -o tools/_bin/wave_simd_probe && tools/_bin/wave_simd_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int LDS_F4 = 133248 / 16;
constexpr int HW_ID_ALL = 4 | (31 << 11);          // hwreg(HW_REG_HW_ID, 0, 32)

__global__ __launch_bounds__(512, 2) void probe(unsigned* out, int nblocks) {
    __shared__ float4 lds[LDS_F4];
    if (threadIdx.x == 0) lds[0] = make_float4(0.f, 0.f, 0.f, 0.f);      // (keeps the allocation)
    __syncthreads();
    const unsigned id = __builtin_amdgcn_s_getreg(HW_ID_ALL);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0 && (int)blockIdx.x < nblocks) out[blockIdx.x * 8 + wave] = id + (unsigned)lds[0].x;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int nblocks = 2 * prop.multiProcessorCount;
    unsigned* d = nullptr;
    CHECK(hipMalloc(&d, (size_t)nblocks * 8 * sizeof(unsigned)));
    CHECK(hipMemset(d, 0xff, (size_t)nblocks * 8 * sizeof(unsigned)));
    hipLaunchKernelGGL(probe, dim3(nblocks), dim3(512), 0, 0, d, nblocks);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned> h((size_t)nblocks * 8);
    CHECK(hipMemcpy(h.data(), d, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    std::map<std::string, int> patterns;
    int paired = 0, same_cu = 0;
    for (int b = 0; b < nblocks; ++b) {
        char s[16];
        bool ok = true, cu = true;
        unsigned seen = 0;
        for (int w = 0; w < 8; ++w) {
            const unsigned id = h[(size_t)b * 8 + w];
            s[w] = (char)('0' + ((id >> 4) & 3));
            cu = cu && ((id >> 8) & 0xff) == ((h[(size_t)b * 8] >> 8) & 0xff);
        }
        s[8] = 0;
        for (int w = 0; w < 4; ++w) { ok = ok && s[w] == s[w + 4]; seen |= 1u << (s[w] - '0'); }
        paired += ok && seen == 15u;
        same_cu += cu;
        ++patterns[s];
    }
    printf("%s, %d CUs, %d blocks of 8 waves\n", prop.name, prop.multiProcessorCount, nblocks);
    printf("blocks whose waves share one CU: %d\n", same_cu);
    printf("blocks with simd(w) == simd(w + 4), w = 0..3, on four different SIMDs: %d of %d\n", paired, nblocks);
    printf("SIMD of waves 0..7 -> blocks:\n");
    for (const auto& kv : patterns) printf("  %s  %d\n", kv.first.c_str(), kv.second);
    return paired == nblocks ? 0 : 2;
}
