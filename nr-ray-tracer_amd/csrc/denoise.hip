// Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a frame and its feature buffers
// (aov.hip).  No reference counterpart.  With a = max(albedo, 1e-3) and D_0 = colour / a, pass
// i = 0 .. K-1 (step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2 .. 2, taps outside the image
// skipped, h = (1/16, 1/4, 3/8, 1/4, 1/16)):
//   e(p, q) = |D_i(p) - D_i(q)|^2 / (sigma_c 2^-i)^2 + |N(p) - N(q)|^2 / sigma_n^2 + (Z(p) - Z(q))^2 / sigma_z^2
//   D_{i+1}(p) = sum_q h[dx] h[dy] exp(-e) D_i(q) / sum_q h[dx] h[dy] exp(-e)
// and the output is D_K a.  No atomics: a pixel's taps are summed in one fixed order by one lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "gpu.hpp"

namespace nrt {

namespace {

constexpr int TW = 32, TH = 8;  // outputs per workgroup: one per lane, a wave = two rows of 32
constexpr int THREADS = TW * TH;
constexpr float ALBEDO_FLOOR = 1e-3f;

struct AtrousParams {
    const float* cin;     // FIRST: the caller's colour; else D_i (3 f32 per pixel)
    const float* albedo;  // FIRST (demodulation) and LAST (remodulation)
    const float* normal;  // FIRST
    const float* depth;   // FIRST
    const float4* gin;    // not FIRST: the guide records (normal.xyz, depth) pass 0 packed
    float4* gout;         // FIRST, when a later pass follows
    float* cout;          // D_{i+1}; LAST: the caller's output
    uint32_t width, height;
    uint32_t pitch;       // lattice pitch g: the tile's points are g pixels apart (1: an image-space tile)
    float kc, kn, kz;     // log2(e) / (sigma_c 2^-i)^2, log2(e) / sigma_n^2, log2(e) / sigma_z^2
};

// One pass.  A workgroup computes TW x TH points of the lattice (x mod g, y mod g) = (lx, ly) and
// stages them plus a halo of 2 T points in LDS, T = s / g: with g = 1 that is an image-space tile
// with its 2 s halo (T = s = 1, 2, 4), with g = s the tile of an independent lattice of the
// step-s pass (T = 1), whose halo stays 2 points however large s is.  Region row-major,
// RW = TW + 4 T wide:
//   sc[3 (v RW + u) + c]  colour, packed as in memory: the staging loop's element e is written to
//                         word e (lane-contiguous, no conflict), and a tap read is word 3 u + const
//                         over the 32 lanes of a row: 3 is odd, so the 32 lanes hit 32 banks;
//   sg[v RW + u]          guide record, one 16-byte read per tap, lane-contiguous.
// Slots outside the image hold zeros and their taps get weight 0 from the coordinate test.
template <int T, bool FIRST, bool LAST>
__global__ void __launch_bounds__(THREADS) atrous_kernel(const AtrousParams p) {
    constexpr int RW = TW + 4 * T, RH = TH + 4 * T, NPIX = RW * RH;
    __shared__ float4 sg[NPIX];
    __shared__ float sc[3 * NPIX];
    const int g = (int)p.pitch, W = (int)p.width, H = (int)p.height;
    const int lx = (int)(blockIdx.x % p.pitch), ly = (int)(blockIdx.y % p.pitch);
    const int tx0 = (int)(blockIdx.x / p.pitch) * TW, ty0 = (int)(blockIdx.y / p.pitch) * TH;  // lattice coordinates
    if (lx + tx0 * g >= W || ly + ty0 * g >= H) return;  // (uniform) a tile past the end of a short lattice
    const int tid = (int)threadIdx.x;
    // region slot (u, v) -> pixel (lx + (tx0 - 2 T + u) g, ly + (ty0 - 2 T + v) g)
    for (int e = tid; e < 3 * NPIX; e += THREADS) {
        const int q = e / 3, c = e - 3 * q, v = q / RW, u = q - v * RW;
        const int x = lx + (tx0 - 2 * T + u) * g, y = ly + (ty0 - 2 * T + v) * g;
        float val = 0.0f;
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const size_t a = ((size_t)y * p.width + (size_t)x) * 3u + (size_t)c;
            val = p.cin[a];
            if constexpr (FIRST) val = val / fmaxf(p.albedo[a], ALBEDO_FLOOR);
        }
        sc[e] = val;
    }
    for (int q = tid; q < NPIX; q += THREADS) {
        const int v = q / RW, u = q - v * RW;
        const int x = lx + (tx0 - 2 * T + u) * g, y = ly + (ty0 - 2 * T + v) * g;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const size_t a = (size_t)y * p.width + (size_t)x;
            if constexpr (FIRST) r = make_float4(p.normal[3 * a], p.normal[3 * a + 1], p.normal[3 * a + 2], p.depth[a]);
            else r = p.gin[a];
        }
        sg[q] = r;
    }
    __syncthreads();
    const int tx = tid % TW, ty = tid / TW;
    const int px = lx + (tx0 + tx) * g, py = ly + (ty0 + ty) * g;
    if (px >= W || py >= H) return;
    const int s = T * g;
    const int cq = (ty + 2 * T) * RW + tx + 2 * T;
    const float4 gp = sg[cq];
    const float c0 = sc[3 * cq], c1 = sc[3 * cq + 1], c2 = sc[3 * cq + 2];
    constexpr float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const bool oky = (unsigned)(py + dy * s) < (unsigned)H;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const bool ok = oky && (unsigned)(px + dx * s) < (unsigned)W;
            const int q = cq + dy * T * RW + dx * T;
            const float4 gq = sg[q];
            const float q0 = sc[3 * q], q1 = sc[3 * q + 1], q2 = sc[3 * q + 2];
            const float d0 = c0 - q0, d1 = c1 - q1, d2 = c2 - q2;
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
            const float e = (d0 * d0 + d1 * d1 + d2 * d2) * p.kc + (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
            // exp(-e) as one v_exp_f32 (the constants carry log2(e))
            const float w = ok ? hk[dx + 2] * hk[dy + 2] * __builtin_amdgcn_exp2f(-e) : 0.0f;
            sw += w;
            a0 += w * q0;
            a1 += w * q1;
            a2 += w * q2;
        }
    }
    // (the centre tap has e = 0: sw >= 9/64)
    float o0 = a0 / sw, o1 = a1 / sw, o2 = a2 / sw;
    const size_t pix = (size_t)py * p.width + (size_t)px;
    if constexpr (LAST) {
        o0 *= fmaxf(p.albedo[3 * pix], ALBEDO_FLOOR);
        o1 *= fmaxf(p.albedo[3 * pix + 1], ALBEDO_FLOOR);
        o2 *= fmaxf(p.albedo[3 * pix + 2], ALBEDO_FLOOR);
    }
    p.cout[3 * pix] = o0;
    p.cout[3 * pix + 1] = o1;
    p.cout[3 * pix + 2] = o2;
    if constexpr (FIRST) {
        if (p.gout) p.gout[pix] = gp;
    }
}

void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

template <int T>
void launch_pass(const AtrousParams& p, bool first, bool last, dim3 grid, hipStream_t stream) {
    if constexpr (T == 1) {  // (pass 0 has step 1)
        if (first && last) hipLaunchKernelGGL((atrous_kernel<1, true, true>), grid, dim3(THREADS), 0, stream, p);
        else if (first) hipLaunchKernelGGL((atrous_kernel<1, true, false>), grid, dim3(THREADS), 0, stream, p);
    }
    if (!first && last) hipLaunchKernelGGL((atrous_kernel<T, false, true>), grid, dim3(THREADS), 0, stream, p);
    else if (!first) hipLaunchKernelGGL((atrous_kernel<T, false, false>), grid, dim3(THREADS), 0, stream, p);
}

// Steps below this take image-space tiles (halo 2 s), steps from it on lattice tiles (halo 2 points);
// at step 1 the two are the same tile.  Knob NRT_ATROUS_LATTICE (1, 2, 4, 8; measurement runs): every
// split gives the same bits.  1024 x 1024 on an MI355X, passes 1 / 2 (steps 2 / 4): image-space tiles
// 33.4 / 41.3 us, lattice tiles 32.2 / 40.1 us (three alternating rounds, spread 0.1 us): lattices from 2.
uint32_t lattice_from() {
    if (const char* e = std::getenv("NRT_ATROUS_LATTICE")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v == 1 || v == 2 || v == 4 || v == 8) return (uint32_t)v;
    }
    return 2u;
}

}  // namespace

struct DenoiseScratch {
    int device = -1;
    size_t pixels = 0;
    float* ping = nullptr;
    float* pong = nullptr;
    float4* guides = nullptr;
};

void gpu_denoise_scratch_free(DenoiseScratch* s) {
    if (!s) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(s->device);
    (void)hipFree(s->ping);
    (void)hipFree(s->pong);
    (void)hipFree(s->guides);
    (void)hipSetDevice(prev);
    delete s;
}

DenoiseScratch* gpu_denoise_scratch(DenoiseScratch* have, size_t pixels, int device) {
    if (have && have->device == device && have->pixels >= pixels) return have;
    gpu_denoise_scratch_free(have);  // (hipFree waits for the device: no pass still reads the old buffers)
    auto* s = new DenoiseScratch();
    s->device = device;
    int prev = 0;
    (void)hipGetDevice(&prev);
    try {
        check(hipSetDevice(device), "hipSetDevice");
        check(hipMalloc((void**)&s->ping, pixels * 3 * sizeof(float)), "hipMalloc(denoise scratch)");
        check(hipMalloc((void**)&s->pong, pixels * 3 * sizeof(float)), "hipMalloc(denoise scratch)");
        check(hipMalloc((void**)&s->guides, pixels * sizeof(float4)), "hipMalloc(denoise scratch)");
        s->pixels = pixels;
    } catch (...) {
        (void)hipSetDevice(prev);
        gpu_denoise_scratch_free(s);
        throw;
    }
    (void)hipSetDevice(prev);
    return s;
}

void gpu_denoise(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                 uint32_t width, uint32_t rows, uint32_t iterations, float sigma_color, float sigma_normal,
                 float sigma_depth, float* out, void* stream_ptr) {
    const size_t pixels = (size_t)width * rows;
    if (!s || s->pixels < pixels) throw std::runtime_error("denoise scratch too small");
    hipStream_t stream = (hipStream_t)stream_ptr;
    int prev = 0;
    (void)hipGetDevice(&prev);
    check(hipSetDevice(s->device), "hipSetDevice");
    const double log2e = 1.4426950408889634;
    const uint32_t lat = lattice_from();
    // a single pass in place would read the halo of pixels other workgroups have already replaced
    const bool alias = iterations == 1 && colour < out + pixels * 3 && out < colour + pixels * 3;
    const float* src = colour;
    float* bufs[2] = {s->ping, s->pong};
    for (uint32_t i = 0; i < iterations; ++i) {
        const bool first = i == 0, last = i + 1 == iterations;
        const uint32_t step = 1u << i, g = step >= lat ? step : 1u;
        AtrousParams p{};
        p.cin = src;
        p.albedo = albedo;
        p.normal = normal;
        p.depth = depth;
        p.gin = s->guides;
        p.gout = last ? nullptr : s->guides;
        p.cout = last && !alias ? out : bufs[i & 1u];
        p.width = width;
        p.height = rows;
        p.pitch = g;
        const double sc = (double)sigma_color / (double)step;
        p.kc = (float)(log2e / (sc * sc));
        p.kn = (float)(log2e / ((double)sigma_normal * sigma_normal));
        p.kz = (float)(log2e / ((double)sigma_depth * sigma_depth));
        // lattice (lx, ly) in the low part of the block index: neighbouring workgroups read the same lines
        const uint32_t lw = (width + g - 1) / g, lh = (rows + g - 1) / g;
        const dim3 grid(((lw + TW - 1) / TW) * g, ((lh + TH - 1) / TH) * g);
        if (step / g == 1) launch_pass<1>(p, first, last, grid, stream);
        else if (step / g == 2) launch_pass<2>(p, first, last, grid, stream);
        else launch_pass<4>(p, first, last, grid, stream);
        src = p.cout;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && alias) e = hipMemcpyAsync(out, src, pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream);
    (void)hipSetDevice(prev);
    check(e, "denoise launch");
}

}  // namespace nrt
