// Adaptive sampling (nrt_render_adaptive, nrt_adaptive_select; formulas: nrt.h).  No reference counterpart.
// Per-pixel state: the running means A, B of two halves of the pixel's samples (3 f32 each) and n, the samples each
// half holds.  Four steps, each a kernel without a wait on another workgroup, without an atomic and with plain
// vector stores only:
//   select   per-pixel relative error from the halves' difference, pooled over the guide-weighted 7 x 7 window
//            (the dual-buffer variance of denoise.hip, per sample); each 32 x 8 tile writes its 256 selection
//            bits, its count and optionally the error
//   scan     exclusive prefix sum of the tile counts by one workgroup, and the total
//   scatter  each tile expands its bits into list[offset[tile] + rank]: tiles in row-major order, pixels
//            row-major inside a tile, so the list is a pure function of the mask
//   merge    folds the list render's new half means A', B' (compact, list order) into A, B and n
// The list launch between scatter and merge is the Philox loop's (kernel.hpp fetch, RenderParams::pixel_list).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <stdexcept>

#include "gpu.hpp"
#include "hip_util.hpp"

namespace nrt {

namespace {

constexpr int TW = 32, TH = 8;  // outputs per workgroup: one per lane, a wave = two rows of 32 (denoise.hip's tile)
constexpr int THREADS = TW * TH;
constexpr int WAVES = THREADS / 64;
constexpr int MASK_WORDS = THREADS / 32;  // a tile's selection bits: bit ty * 32 + tx
constexpr int VR = 3;                     // the window's radius
constexpr int VW = TW + 2 * VR, VH = TH + 2 * VR;  // 38 x 14 slots
constexpr int VPIX = VW * VH;
constexpr float ALBEDO_FLOOR = 1e-3f;
constexpr double LOG2E = 1.4426950408889634;

struct SelectParams {
    const float* a;       // half means, 3 f32 per pixel
    const float* b;
    const uint32_t* n;    // samples per half
    const float* albedo;
    const float* normal;
    const float* depth;
    uint32_t width, height;
    uint32_t level;       // only pixels with n == level are candidates
    float threshold;
    float kn, kz;         // log2(e) / sigma_n^2, log2(e) / sigma_z^2
    uint32_t* mask;       // MASK_WORDS words per tile
    uint32_t* counts;     // one per tile
    float* err;           // 1 f32 per pixel, or null
};

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }
__device__ __forceinline__ float lum(float r, float g, float b) {
    return fmaf(0.2126f, r, fmaf(0.7152f, g, 0.0722f * b));
}
__device__ __forceinline__ float floor_albedo(const SelectParams& p, size_t i) { return fmaxf(p.albedo[i], ALBEDO_FLOOR); }

// One tile: 32 x 8 pixels and a halo of 3 staged in LDS, 38 x 14 slots of one word v = n delta^2 (the slot's
// per-sample variance estimate, delta = lum((A - B) / a) / 2) and one 16-byte guide record (normal.xyz, depth),
// 10 640 B.  Consecutive lanes read consecutive words / records at every tap: no bank conflict.  A lane sums its 49
// taps in one fixed order, rows of taps not unrolled, the 7 taps of a row unrolled.  Slots outside the image hold
// zeros and their taps weigh 0.  Every lane stays to the end: the ballot and the count need the whole workgroup.
__global__ void __launch_bounds__(THREADS) adaptive_select_kernel(const SelectParams p) {
    __shared__ float4 sg[VPIX];
    __shared__ float sv[VPIX];
    __shared__ uint32_t wave_count[WAVES];
    const int W = (int)p.width, H = (int)p.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
    for (int q = tid; q < VPIX; q += THREADS) {
        const int v = q / VW, u = q - v * VW;
        const int x = tx0 - VR + u, y = ty0 - VR + v;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float word = 0.0f;
        if (in_range(x, W) && in_range(y, H)) {
            const size_t i = (size_t)y * p.width + (size_t)x;
            r = make_float4(p.normal[3 * i], p.normal[3 * i + 1], p.normal[3 * i + 2], p.depth[i]);
            const float d = 0.5f * lum((p.a[3 * i] - p.b[3 * i]) / floor_albedo(p, 3 * i),
                                       (p.a[3 * i + 1] - p.b[3 * i + 1]) / floor_albedo(p, 3 * i + 1),
                                       (p.a[3 * i + 2] - p.b[3 * i + 2]) / floor_albedo(p, 3 * i + 2));
            word = (float)p.n[i] * (d * d);
        }
        sg[q] = r;
        sv[q] = word;
    }
    __syncthreads();
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    bool select = false;
    if (px < W && py < H) {
        const int cq = (ty + VR) * VW + tx + VR;
        const float4 gp = sg[cq];
        float sw = 0.0f, s2 = 0.0f;
#pragma unroll 1
        for (int dy = -VR; dy <= VR; ++dy) {
            const bool oky = in_range(py + dy, H);
#pragma unroll
            for (int dx = -VR; dx <= VR; ++dx) {
                const bool ok = oky && in_range(px + dx, W);
                const int q = cq + dy * VW + dx;
                const float4 gq = sg[q];
                const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
                const float e = (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
                const float w = ok ? __builtin_amdgcn_exp2f(-e) : 0.0f;
                sw += w;
                s2 += w * sv[q];
            }
        }
        // (the centre tap has w = 1: sw >= 1)
        const size_t i = (size_t)py * p.width + (size_t)px;
        const uint32_t np = p.n[i];
        const float var = (s2 / sw) / (float)np;  // of p's mean over its 2 n samples
        const float mean = lum(((p.a[3 * i] + p.b[3 * i]) * 0.5f) / floor_albedo(p, 3 * i),
                               ((p.a[3 * i + 1] + p.b[3 * i + 1]) * 0.5f) / floor_albedo(p, 3 * i + 1),
                               ((p.a[3 * i + 2] + p.b[3 * i + 2]) * 0.5f) / floor_albedo(p, 3 * i + 2));
        const float err = sqrtf(var) / (mean + 0.01f);
        if (p.err) p.err[i] = err;
        select = np == p.level && err >= p.threshold;  // (threshold 0 refines a pixel whose halves agree exactly)
    }
    const unsigned long long bits = __ballot(select);  // bit = lane: row-major inside the wave's two rows
    const int wave = tid >> 6;
    const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
    if ((tid & 63) == 0) {
        p.mask[(size_t)tile * MASK_WORDS + 2 * wave] = (uint32_t)bits;
        p.mask[(size_t)tile * MASK_WORDS + 2 * wave + 1] = (uint32_t)(bits >> 32);
        wave_count[wave] = (uint32_t)__popcll(bits);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        for (int w = 0; w < WAVES; ++w) c += wave_count[w];
        p.counts[tile] = c;
    }
}

// Exclusive scan of the tile counts by one workgroup: THREADS counts per round, a wave prefix sum by lane shifts,
// the four wave sums through LDS, the rounds' carry in a register.  offsets[i] = sum of counts[0 .. i), *total = all.
__global__ void __launch_bounds__(THREADS) adaptive_scan_kernel(const uint32_t* counts, uint32_t tiles, uint32_t* offsets,
                                                                uint32_t* total) {
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += THREADS) {  // (uniform trip count: every lane meets the barriers)
        const uint32_t i = base + tid;
        const uint32_t c = i < tiles ? counts[i] : 0u;
        uint32_t s = c;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(s, d);
            s += lane >= d ? t : 0u;
        }
        if (lane == 63u) wave_sum[wave] = s;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
            before += w < wave ? wave_sum[w] : 0u;
            all += wave_sum[w];
        }
        if (i < tiles) offsets[i] = carry + before + s - c;
        carry += all;
        __syncthreads();  // wave_sum is rewritten by the next round
    }
    if (tid == 0) *total = carry;
}

// A tile's bits into the list: a lane's rank is the set bits below it in its wave's 64 (mbcnt) plus the earlier
// waves' counts; entries at or past `cap` are dropped (the total says how many there were).
__global__ void __launch_bounds__(THREADS) adaptive_scatter_kernel(const uint32_t* mask, const uint32_t* offsets,
                                                                   uint32_t width, uint32_t* list, uint32_t cap) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t* m = mask + (size_t)tile * MASK_WORDS;
    uint32_t base = offsets[tile];
    for (uint32_t w = 0; w < wave; ++w) base += (uint32_t)__popc(m[2 * w]) + (uint32_t)__popc(m[2 * w + 1]);
    const uint32_t lo = m[2 * wave], hi = m[2 * wave + 1];
    const bool set = (((lane < 32u ? lo : hi) >> (lane & 31u)) & 1u) != 0u;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    const uint32_t x = blockIdx.x * TW + tid % TW, y = blockIdx.y * TH + tid / TW;
    const uint32_t at = base + rank;
    if (set && at < cap) list[at] = y * width + x;  // (a set bit is a pixel of the image: select kernel)
}

// List entry i, pixel p, m new samples per half: A[p] = (n A[p] + m A'[i]) / (n + m) in f64, rounded once; n[p] += m.
// The list's pixels are distinct, so no two lanes write one pixel.
__global__ void __launch_bounds__(THREADS) adaptive_merge_kernel(const uint32_t* list, uint32_t count, uint32_t m, float* a,
                                                                 float* b, uint32_t* n, const float* a_new,
                                                                 const float* b_new) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= count) return;
    const size_t p = list[i];
    const uint32_t np = n[p];
    const double wn = (double)np, wm = (double)m, sum = (double)(np + m);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[3 * p + c] = (float)((wn * (double)a[3 * p + c] + wm * (double)a_new[3 * (size_t)i + c]) / sum);
        b[3 * p + c] = (float)((wn * (double)b[3 * p + c] + wm * (double)b_new[3 * (size_t)i + c]) / sum);
    }
    n[p] = np + m;
}

__global__ void __launch_bounds__(THREADS) adaptive_fill_kernel(uint32_t* n, size_t pixels, uint32_t value) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < pixels) n[i] = value;
}

// out = (A + B) / 2 per channel in f32, samples = 2 n
__global__ void __launch_bounds__(THREADS) adaptive_finish_kernel(const float* a, const float* b, const uint32_t* n,
                                                                  size_t pixels, float* out, uint32_t* samples) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= pixels) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (a[3 * i + c] + b[3 * i + c]) * 0.5f;
    samples[i] = 2u * n[i];
}

dim3 tile_grid(uint32_t width, uint32_t rows) { return dim3((width + TW - 1) / TW, (rows + TH - 1) / TH); }
uint32_t linear_blocks(size_t n) { return (uint32_t)((n + THREADS - 1) / THREADS); }

}  // namespace

struct AdaptiveScratch {
    int device = -1;
    size_t pixels = 0;
    AdaptiveBuffers buf{};
    uint32_t* mask = nullptr;     // MASK_WORDS per tile, for at most pixels one-pixel tiles' worth: see below
    uint32_t* counts = nullptr;   // per tile
    uint32_t* offsets = nullptr;  // per tile, then the total
    uint32_t* host_count = nullptr;  // pinned: the total's read-back
    size_t tiles = 0;
};

// Tiles of a frame of `pixels` pixels, whatever its shape: a frame w x h has ceil(w / 32) ceil(h / 8) tiles, at most
// (w / 32 + 1) (h / 8 + 1) <= pixels / 256 + w / 32 + h / 8 + 1 <= pixels / 256 + pixels / 8 + 2 (w, h <= pixels).
static size_t max_tiles(size_t pixels) { return pixels / 256 + pixels / 8 + 2; }

void gpu_adaptive_scratch_free(AdaptiveScratch* s) {
    if (!s) return;
    try {
        DeviceGuard guard(s->device);
        const AdaptiveBuffers& b = s->buf;
        for (void* p : std::initializer_list<void*>{b.a, b.b, b.n, b.list, b.a_new, b.b_new, b.albedo, b.normal, b.depth,
                                                    s->mask, s->counts, s->offsets})
            if (p) (void)hipFree(p);
        if (s->host_count) (void)hipHostFree(s->host_count);
    } catch (...) {  // (the device cannot be made current: nothing of it is left to free)
    }
    delete s;
}

AdaptiveScratch* gpu_adaptive_scratch(AdaptiveScratch* have, size_t pixels, int device) {
    if (have && have->device == device && have->pixels >= pixels) return have;
    gpu_adaptive_scratch_free(have);  // (hipFree waits for the device: no kernel still reads the old buffers)
    std::unique_ptr<AdaptiveScratch, decltype(&gpu_adaptive_scratch_free)> s(new AdaptiveScratch(), gpu_adaptive_scratch_free);
    s->device = device;
    DeviceGuard guard(device);
    auto f32s = [&](float*& p, size_t n) { check(hipMalloc((void**)&p, n * sizeof(float)), "hipMalloc(adaptive scratch)"); };
    auto u32s = [&](uint32_t*& p, size_t n) { check(hipMalloc((void**)&p, n * sizeof(uint32_t)), "hipMalloc(adaptive scratch)"); };
    AdaptiveBuffers& b = s->buf;
    f32s(b.a, 3 * pixels);
    f32s(b.b, 3 * pixels);
    u32s(b.n, pixels);
    u32s(b.list, pixels);
    f32s(b.a_new, 3 * pixels);
    f32s(b.b_new, 3 * pixels);
    f32s(b.albedo, 3 * pixels);
    f32s(b.normal, 3 * pixels);
    f32s(b.depth, pixels);
    s->tiles = max_tiles(pixels);
    u32s(s->mask, s->tiles * MASK_WORDS);
    u32s(s->counts, s->tiles);
    u32s(s->offsets, s->tiles + 1);
    check(hipHostMalloc((void**)&s->host_count, sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc(adaptive count)");
    s->pixels = pixels;
    return s.release();
}

AdaptiveBuffers gpu_adaptive_buffers(const AdaptiveScratch* s) { return s->buf; }

void gpu_adaptive_select(AdaptiveScratch* s, const float* a, const float* b, const uint32_t* n, const float* albedo,
                         const float* normal, const float* depth, uint32_t width, uint32_t rows, uint32_t level,
                         float threshold, float sigma_normal, float sigma_depth, uint32_t* list, uint32_t cap,
                         uint32_t* total, float* err, void* stream_ptr) {
    const dim3 grid = tile_grid(width, rows);
    const size_t tiles = (size_t)grid.x * grid.y;
    if (!s || s->pixels < (size_t)width * rows || s->tiles < tiles) throw std::runtime_error("adaptive scratch too small");
    hipStream_t stream = (hipStream_t)stream_ptr;
    DeviceGuard guard(s->device);
    SelectParams p{};
    p.a = a;
    p.b = b;
    p.n = n;
    p.albedo = albedo;
    p.normal = normal;
    p.depth = depth;
    p.width = width;
    p.height = rows;
    p.level = level;
    p.threshold = threshold;
    p.kn = (float)(LOG2E / ((double)sigma_normal * sigma_normal));
    p.kz = (float)(LOG2E / ((double)sigma_depth * sigma_depth));
    p.mask = s->mask;
    p.counts = s->counts;
    p.err = err;
    hipLaunchKernelGGL(adaptive_select_kernel, grid, dim3(THREADS), 0, stream, p);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(THREADS), 0, stream, s->counts, (uint32_t)tiles, s->offsets,
                       total ? total : s->offsets + s->tiles);
    hipLaunchKernelGGL(adaptive_scatter_kernel, grid, dim3(THREADS), 0, stream, s->mask, s->offsets, width, list, cap);
    check(hipGetLastError(), "adaptive select launch");
}

uint32_t gpu_adaptive_count(AdaptiveScratch* s, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    DeviceGuard guard(s->device);
    check(hipMemcpyAsync(s->host_count, s->offsets + s->tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
          "adaptive count read-back");
    check(hipStreamSynchronize(stream), "adaptive count read-back");
    return *s->host_count;
}

void gpu_adaptive_merge(AdaptiveScratch* s, uint32_t count, uint32_t m, void* stream_ptr) {
    if (!count) return;
    DeviceGuard guard(s->device);
    const AdaptiveBuffers& b = s->buf;
    hipLaunchKernelGGL(adaptive_merge_kernel, dim3(linear_blocks(count)), dim3(THREADS), 0, (hipStream_t)stream_ptr, b.list,
                       count, m, b.a, b.b, b.n, b.a_new, b.b_new);
    check(hipGetLastError(), "adaptive merge launch");
}

void gpu_adaptive_fill(AdaptiveScratch* s, size_t pixels, uint32_t value, void* stream_ptr) {
    DeviceGuard guard(s->device);
    hipLaunchKernelGGL(adaptive_fill_kernel, dim3(linear_blocks(pixels)), dim3(THREADS), 0, (hipStream_t)stream_ptr, s->buf.n,
                       pixels, value);
    check(hipGetLastError(), "adaptive fill launch");
}

void gpu_adaptive_finish(AdaptiveScratch* s, size_t pixels, float* out, uint32_t* samples, void* stream_ptr) {
    DeviceGuard guard(s->device);
    const AdaptiveBuffers& b = s->buf;
    hipLaunchKernelGGL(adaptive_finish_kernel, dim3(linear_blocks(pixels)), dim3(THREADS), 0, (hipStream_t)stream_ptr, b.a, b.b,
                       b.n, pixels, out, samples);
    check(hipGetLastError(), "adaptive finish launch");
}

}  // namespace nrt
