// Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a frame and its feature buffers
// (aov.hip).  No reference counterpart.  With a = max(albedo, 1e-3) and D_0 = colour / a, pass
// i = 0 .. K-1 (step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2 .. 2, taps outside the image
// skipped, h = (1/16, 1/4, 3/8, 1/4, 1/16)):
//   e(p, q) = |D_i(p) - D_i(q)|^2 / (sigma_c 2^-i)^2 + |N(p) - N(q)|^2 / sigma_n^2 + (Z(p) - Z(q))^2 / sigma_z^2
//   D_{i+1}(p) = sum_q h[dx] h[dy] exp(-e) D_i(q) / sum_q h[dx] h[dy] exp(-e)
// and the output is D_K a.  No atomics: a pixel's taps are summed in one fixed order by one lane.
//
// Variance-guided variant (SVGF's spatial filter, Schied et al. 2017; second half of this file): the
// colour term above gives way to a luminance term scaled by the local standard deviation, which a
// 7 x 7 moments kernel estimates from the frame and every pass carries along.  Formula: nrt.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

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
    size_t rec_bytes = 0;  // per pixel of ping and pong: 12 (packed colour) or 16 (colour and variance)
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

DenoiseScratch* gpu_denoise_scratch(DenoiseScratch* have, size_t pixels, int device, size_t rec_bytes) {
    if (have && have->device == device && have->pixels >= pixels && have->rec_bytes >= rec_bytes) return have;
    gpu_denoise_scratch_free(have);  // (hipFree waits for the device: no pass still reads the old buffers)
    auto* s = new DenoiseScratch();
    s->device = device;
    int prev = 0;
    (void)hipGetDevice(&prev);
    try {
        check(hipSetDevice(device), "hipSetDevice");
        check(hipMalloc((void**)&s->ping, pixels * rec_bytes), "hipMalloc(denoise scratch)");
        check(hipMalloc((void**)&s->pong, pixels * rec_bytes), "hipMalloc(denoise scratch)");
        check(hipMalloc((void**)&s->guides, pixels * sizeof(float4)), "hipMalloc(denoise scratch)");
        s->pixels = pixels;
        s->rec_bytes = rec_bytes;
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
    if (!s || s->pixels < pixels || s->rec_bytes < 3 * sizeof(float)) throw std::runtime_error("denoise scratch too small");
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

// ---- variance-guided filter: 7 x 7 moments kernel, then K passes over (colour, variance) records
namespace {

constexpr int VR = 3;                                   // the moments window's radius
constexpr int VW = TW + 2 * VR, VH = TH + 2 * VR;       // 38 x 14 slots
constexpr int VPIX = VW * VH;

struct VgParams {
    const float* colour;  // moments kernel: the caller's colour
    const float* albedo;  // moments kernel (demodulation) and LAST (remodulation)
    const float* normal;  // moments kernel
    const float* depth;   // moments kernel
    const float4* rin;    // passes: (D_i.rgb, Var_i)
    const float4* gin;    // passes: the guide records (normal.xyz, depth) the moments kernel packed
    float4* rout;         // moments kernel: (D_0, Var_0); passes but LAST: (D_{i+1}, Var_{i+1})
    float4* gout;         // moments kernel
    float* cout;          // LAST: the caller's output, 3 f32 per pixel
    float* vout;          // LAST: the caller's variance buffer, 1 f32 per pixel, or null
    uint32_t width, height;
    uint32_t pitch;       // as AtrousParams
    float sigma_l, kn, kz;  // sigma_l, log2(e) / sigma_n^2, log2(e) / sigma_z^2
};

__device__ __forceinline__ float lum(float r, float g, float b) {
    return fmaf(0.2126f, r, fmaf(0.7152f, g, 0.0722f * b));
}

// Var_0 and the records of the passes.  A workgroup computes 32 x 8 pixels and stages them plus a halo
// of 3 in LDS, 38 x 14 slots: one word of demodulated luminance and one 16-byte guide record each
// (4 B + 16 B, 10.6 KB).  Consecutive lanes read consecutive words / records at every tap, so neither
// array has a bank conflict.  Each lane sums its 49 taps in one fixed order; the luminance is shifted
// by the centre's, so the two moments stay of the noise's size and their difference does not cancel.
// (The two halves below are shared with temporal_kernel.)
__device__ __forceinline__ void vg_stage(const VgParams& p, float4* sg, float* sl, int tx0, int ty0, int tid) {
    const int W = (int)p.width, H = (int)p.height;
    for (int q = tid; q < VPIX; q += THREADS) {
        const int v = q / VW, u = q - v * VW;
        const int x = tx0 - VR + u, y = ty0 - VR + v;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float l = 0.0f;
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const size_t a = (size_t)y * p.width + (size_t)x;
            r = make_float4(p.normal[3 * a], p.normal[3 * a + 1], p.normal[3 * a + 2], p.depth[a]);
            l = lum(p.colour[3 * a] / fmaxf(p.albedo[3 * a], ALBEDO_FLOOR),
                    p.colour[3 * a + 1] / fmaxf(p.albedo[3 * a + 1], ALBEDO_FLOOR),
                    p.colour[3 * a + 2] / fmaxf(p.albedo[3 * a + 2], ALBEDO_FLOOR));
        }
        sg[q] = r;
        sl[q] = l;
    }
}

// Var_0 of the pixel (px, py) at region slot cq
__device__ __forceinline__ float vg_var0(const VgParams& p, const float4* sg, const float* sl, int cq, int px, int py) {
    const int W = (int)p.width, H = (int)p.height;
    const float4 gp = sg[cq];
    const float lp = sl[cq];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
    for (int dy = -VR; dy <= VR; ++dy) {
        const bool oky = (unsigned)(py + dy) < (unsigned)H;
#pragma unroll
        for (int dx = -VR; dx <= VR; ++dx) {
            const bool ok = oky && (unsigned)(px + dx) < (unsigned)W;
            const int q = cq + dy * VW + dx;
            const float4 gq = sg[q];
            const float d = sl[q] - lp;
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
            const float e = (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
            const float w = ok ? __builtin_amdgcn_exp2f(-e) : 0.0f;
            sw += w;
            s1 += w * d;
            s2 += w * d * d;
        }
    }
    // (the centre tap has w = 1: sw >= 1)
    const float m1 = s1 / sw, m2 = s2 / sw;
    return fmaxf(0.0f, m2 - m1 * m1);
}

__global__ void __launch_bounds__(THREADS) vg_moments_kernel(const VgParams p) {
    __shared__ float4 sg[VPIX];
    __shared__ float sl[VPIX];
    const int W = (int)p.width, H = (int)p.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
    vg_stage(p, sg, sl, tx0, ty0, tid);
    __syncthreads();
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    if (px >= W || py >= H) return;
    const int cq = (ty + VR) * VW + tx + VR;
    const float var0 = vg_var0(p, sg, sl, cq, px, py);
    const size_t pix = (size_t)py * p.width + (size_t)px;
    // the lane's own D_0 again from memory (the lines the staging loop just read): the same divisions,
    // so the luminance of this record is the staged one
    p.rout[pix] = make_float4(p.colour[3 * pix] / fmaxf(p.albedo[3 * pix], ALBEDO_FLOOR),
                              p.colour[3 * pix + 1] / fmaxf(p.albedo[3 * pix + 1], ALBEDO_FLOOR),
                              p.colour[3 * pix + 2] / fmaxf(p.albedo[3 * pix + 2], ALBEDO_FLOOR), var0);
    p.gout[pix] = sg[cq];
}

// One pass: atrous_kernel's tile (lattice pitch g, taps T points apart, halo 2 T points) over 16-byte
// (D.rgb, Var) records instead of the packed colour.  Region row-major, RW = TW + 4 T wide:
//   sr[v RW + u]  colour and variance, one 16-byte read per tap;
//   sg[v RW + u]  guide record, one 16-byte read per tap.
// Both are read by the 32 lanes of a row at consecutive slots (T = 1: 16 consecutive bytes per lane,
// 512 contiguous bytes per row of lanes, the access a b128 read serves at full rate; the packed
// colour's odd-stride argument has nothing left to do).  With T = 2 / 4 (image-space tiles of the steps
// 2 / 4, measurement runs only) the lanes are 32 / 64 bytes apart and the reads take 2 / 4 times as long.
// sigma(p), the 3 x 3 distance-1 prefilter of Var_i, needs pixels no lattice tile holds: the lane
// reads the nine .w words from memory before the staging loop, so that their latency runs under it.
// At pitch 1 they are the lines the workgroup stages anyway, at pitch g those the g^2 - 1 neighbouring
// lattices' workgroups (adjacent block indices) stage.
template <int T, bool LAST>
__global__ void __launch_bounds__(THREADS) vg_atrous_kernel(const VgParams p) {
    constexpr int RW = TW + 4 * T, RH = TH + 4 * T, NPIX = RW * RH;
    __shared__ float4 sr[NPIX];
    __shared__ float4 sg[NPIX];
    const int g = (int)p.pitch, W = (int)p.width, H = (int)p.height;
    const int lx = (int)(blockIdx.x % p.pitch), ly = (int)(blockIdx.y % p.pitch);
    const int tx0 = (int)(blockIdx.x / p.pitch) * TW, ty0 = (int)(blockIdx.y / p.pitch) * TH;  // lattice coordinates
    if (lx + tx0 * g >= W || ly + ty0 * g >= H) return;  // (uniform) a tile past the end of a short lattice
    const int tid = (int)threadIdx.x;
    const int tx = tid % TW, ty = tid / TW;
    const int px = lx + (tx0 + tx) * g, py = ly + (ty0 + ty) * g;
    const bool mine = px < W && py < H;
    constexpr float g3[3] = {0.25f, 0.5f, 0.25f};
    float pv = 0.0f, pk = 0.0f;
    if (mine) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = px + dx, y = py + dy;
                if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
                    pv += g3[dx + 1] * g3[dy + 1] * p.rin[(size_t)y * p.width + (size_t)x].w;
                    pk += g3[dx + 1] * g3[dy + 1];
                }
            }
        }
    }
    // region slot (u, v) -> pixel (lx + (tx0 - 2 T + u) g, ly + (ty0 - 2 T + v) g)
    for (int q = tid; q < NPIX; q += THREADS) {
        const int v = q / RW, u = q - v * RW;
        const int x = lx + (tx0 - 2 * T + u) * g, y = ly + (ty0 - 2 * T + v) * g;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f), k = r;
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const size_t a = (size_t)y * p.width + (size_t)x;
            r = p.rin[a];
            k = p.gin[a];
        }
        sr[q] = r;
        sg[q] = k;
    }
    __syncthreads();
    if (!mine) return;
    const int s = T * g;
    const int cq = (ty + 2 * T) * RW + tx + 2 * T;
    const float4 gp = sg[cq], rp = sr[cq];
    const float lp = lum(rp.x, rp.y, rp.z);
    // log2(e) / (sigma_l sigma(p) + 1e-6): the centre tap's own weight 1/4 keeps pk >= 1/4
    const float kl = 1.4426950408889634f / (p.sigma_l * sqrtf(pv / pk) + 1e-6f);
    constexpr float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, av = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const bool oky = (unsigned)(py + dy * s) < (unsigned)H;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const bool ok = oky && (unsigned)(px + dx * s) < (unsigned)W;
            const int q = cq + dy * T * RW + dx * T;
            const float4 gq = sg[q], rq = sr[q];
            const float dl = fabsf(lp - lum(rq.x, rq.y, rq.z));
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
            const float e = dl * kl + (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
            const float w = ok ? hk[dx + 2] * hk[dy + 2] * __builtin_amdgcn_exp2f(-e) : 0.0f;
            sw += w;
            a0 += w * rq.x;
            a1 += w * rq.y;
            a2 += w * rq.z;
            av += w * w * rq.w;
        }
    }
    // (the centre tap has e = 0: sw >= 9/64)
    float o0 = a0 / sw, o1 = a1 / sw, o2 = a2 / sw;
    const float ov = av / (sw * sw);
    const size_t pix = (size_t)py * p.width + (size_t)px;
    if constexpr (LAST) {
        p.cout[3 * pix] = o0 * fmaxf(p.albedo[3 * pix], ALBEDO_FLOOR);
        p.cout[3 * pix + 1] = o1 * fmaxf(p.albedo[3 * pix + 1], ALBEDO_FLOOR);
        p.cout[3 * pix + 2] = o2 * fmaxf(p.albedo[3 * pix + 2], ALBEDO_FLOOR);
        if (p.vout) p.vout[pix] = ov;
    } else {
        p.rout[pix] = make_float4(o0, o1, o2, ov);
    }
}

template <int T>
void launch_vg_pass(const VgParams& p, bool last, dim3 grid, hipStream_t stream) {
    if (last) hipLaunchKernelGGL((vg_atrous_kernel<T, true>), grid, dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((vg_atrous_kernel<T, false>), grid, dim3(THREADS), 0, stream, p);
}

// Enqueue passes 0 .. K-1 (p filled but rin, rout, pitch): pass i reads chain[i] and, unless it is the
// last, writes chain[i + 1].
void enqueue_vg_passes(VgParams p, uint32_t iterations, float4* const* chain, hipStream_t stream) {
    const uint32_t lat = lattice_from();
    for (uint32_t i = 0; i < iterations; ++i) {
        const uint32_t step = 1u << i, g = step >= lat ? step : 1u;
        p.rin = chain[i];
        p.rout = chain[i + 1];
        p.pitch = g;
        const uint32_t lw = (p.width + g - 1) / g, lh = (p.height + g - 1) / g;
        const dim3 grid(((lw + TW - 1) / TW) * g, ((lh + TH - 1) / TH) * g);
        if (step / g == 1) launch_vg_pass<1>(p, i + 1 == iterations, grid, stream);
        else if (step / g == 2) launch_vg_pass<2>(p, i + 1 == iterations, grid, stream);
        else launch_vg_pass<4>(p, i + 1 == iterations, grid, stream);
    }
}

// (the fields every vg launch shares)
VgParams vg_params(const float* colour, const float* albedo, const float* normal, const float* depth, uint32_t width,
                   uint32_t rows, float sigma_luminance, float sigma_normal, float sigma_depth, float* out,
                   float* out_variance) {
    const double log2e = 1.4426950408889634;
    VgParams p{};
    p.colour = colour;
    p.albedo = albedo;
    p.normal = normal;
    p.depth = depth;
    p.cout = out;
    p.vout = out_variance;
    p.width = width;
    p.height = rows;
    p.sigma_l = sigma_luminance;
    p.kn = (float)(log2e / ((double)sigma_normal * sigma_normal));
    p.kz = (float)(log2e / ((double)sigma_depth * sigma_depth));
    return p;
}

}  // namespace

// The moments kernel reads the caller's colour and no pass does (the last one reads the albedo), so
// out == colour needs no copy for any K.
void gpu_denoise_vg(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                    uint32_t width, uint32_t rows, uint32_t iterations, float sigma_luminance, float sigma_normal,
                    float sigma_depth, float* out, float* out_variance, void* stream_ptr) {
    const size_t pixels = (size_t)width * rows;
    if (!s || s->pixels < pixels || s->rec_bytes < sizeof(float4)) throw std::runtime_error("denoise scratch too small");
    hipStream_t stream = (hipStream_t)stream_ptr;
    int prev = 0;
    (void)hipGetDevice(&prev);
    check(hipSetDevice(s->device), "hipSetDevice");
    float4* const b0 = (float4*)s->ping;
    float4* const b1 = (float4*)s->pong;
    float4* const chain[6] = {b0, b1, b0, b1, b0, b1};
    VgParams p = vg_params(colour, albedo, normal, depth, width, rows, sigma_luminance, sigma_normal, sigma_depth, out,
                           out_variance);
    p.gin = s->guides;
    p.gout = s->guides;
    p.rout = b0;
    hipLaunchKernelGGL(vg_moments_kernel, dim3((width + TW - 1) / TW, (rows + TH - 1) / TH), dim3(THREADS), 0, stream, p);
    enqueue_vg_passes(p, iterations, chain, stream);
    const hipError_t e = hipGetLastError();
    (void)hipSetDevice(prev);
    check(e, "denoise_vg launch");
}

// ---- temporal accumulation (SVGF's temporal half): one kernel in the moments kernel's place, then
//      the passes above unchanged.  Formula: nrt.h (nrt_denoise_temporal).
namespace {

struct TemporalParams {
    VgParams v;          // colour, albedo, normal, depth, width, height, kn, kz; rout = (I, V), gout = this frame's guides
    const float4* pg;    // previous frame: guide records (N', Z')
    const float4* ph;    // previous frame: (H'.rgb, .w unused here: the first pass's variance)
    const float4* pm;    // previous frame: (m1', m2', n', 0)
    float4* mout;        // this frame's (m1, m2, n, 0)
    uint32_t have_prev;  // 0: every pixel's history is invalid (first frame, after a reset)
    float c0[3], du[3], dv[3];  // this camera: top_left - look_from, pixel_delta_u, pixel_delta_v
    float dl[3];         // look_from - look_from'
    float t[3];          // M'^-1 (look_from - look_from')
    float e[9];          // M'^-1 (M - M'), row-major: zero for equal cameras
    float alpha_min, tau_z, tau_n;
};

// A workgroup computes 32 x 8 pixels.  Before the barrier every lane reads its own pixel, reprojects
// it and issues the loads of its four taps, three 16-byte records each (guide, H', moments) from the
// previous frame's buffers: neighbouring lanes reproject to neighbouring pixels, so a row of lanes
// gathers from one or two rows of records, and the loads' latency runs under the staging of the
// 38 x 14 region (vg_stage: the moments kernel's, the same LDS layout and conflict-free reads).
//
// The reprojection is evaluated relative to the pixel itself.  With k = Z / |d| and
// (A, B, Cc) = M'^-1 r = k (x, y, 1) + k E (x, y, 1) + t,  E = M'^-1 (M - M'),  t = M'^-1 (look_from - look_from'),
// and w = 1 / k:
//   c = 1 + E_2 . (x, y, 1) + w t_2                     (= Cc / k, the same sign)
//   u - x = (E_0 . (x, y, 1) + w t_0 - x (c - 1)) / c,  v - y likewise with E_1, t_1
// so the rounding error of (u, v) is a few ulps of the motion, not of the pixel coordinate, and equal
// cameras (E = 0, t = 0) give u = x, v = y exactly.  The host computes E and t in f64.
//
// After the barrier: tap tests, the blend, and Var_0 (vg_var0, 49 LDS taps) only in waves where the
// ballot finds a lane with n < 4: a scalar branch, so a steady-state wave skips the loop whole.
__global__ void __launch_bounds__(THREADS) temporal_kernel(const TemporalParams p) {
    __shared__ float4 sg[VPIX];
    __shared__ float sl[VPIX];
    const int W = (int)p.v.width, H = (int)p.v.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    const bool mine = px < W && py < H;
    const size_t pix = mine ? (size_t)py * p.v.width + (size_t)px : 0;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 tg[4] = {zero, zero, zero, zero}, th[4] = {zero, zero, zero, zero}, tm[4] = {zero, zero, zero, zero};
    float4 gp = zero;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, fx = 0.0f, fy = 0.0f, zr = 0.0f;
    bool reproj = false;
    if (mine) {
        gp = make_float4(p.v.normal[3 * pix], p.v.normal[3 * pix + 1], p.v.normal[3 * pix + 2], p.v.depth[pix]);
        d0 = p.v.colour[3 * pix] / fmaxf(p.v.albedo[3 * pix], ALBEDO_FLOOR);
        d1 = p.v.colour[3 * pix + 1] / fmaxf(p.v.albedo[3 * pix + 1], ALBEDO_FLOOR);
        d2 = p.v.colour[3 * pix + 2] / fmaxf(p.v.albedo[3 * pix + 2], ALBEDO_FLOOR);
        if (p.have_prev && gp.w > 0.0f) {
            const float x = (float)px, y = (float)py;
            const float r0 = fmaf(y, p.dv[0], fmaf(x, p.du[0], p.c0[0]));
            const float r1 = fmaf(y, p.dv[1], fmaf(x, p.du[1], p.c0[1]));
            const float r2 = fmaf(y, p.dv[2], fmaf(x, p.du[2], p.c0[2]));
            const float len = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
            const float k = gp.w / len, w = len / gp.w;
            const float q0 = p.dl[0] + k * r0, q1 = p.dl[1] + k * r1, q2 = p.dl[2] + k * r2;  // r = P - look_from'
            zr = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
            const float e0 = fmaf(w, p.t[0], fmaf(y, p.e[1], fmaf(x, p.e[0], p.e[2])));
            const float e1 = fmaf(w, p.t[1], fmaf(y, p.e[4], fmaf(x, p.e[3], p.e[5])));
            const float e2 = fmaf(w, p.t[2], fmaf(y, p.e[7], fmaf(x, p.e[6], p.e[8])));
            const float c = 1.0f + e2;
            const float mu = (e0 - x * e2) / c, mv = (e1 - y * e2) / c;  // u - x, v - y
            const float fu = floorf(mu), fv = floorf(mv);
            const float bx = x + fu, by = y + fv;  // the first tap, still as floats: NaN and far-off motion fail here
            if (c > 0.0f && bx >= -1.0f && bx <= (float)(W - 1) && by >= -1.0f && by <= (float)(H - 1)) {
                reproj = true;
                fx = mu - fu;
                fy = mv - fv;
                const int ix = (int)bx, iy = (int)by;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if ((unsigned)(ix + i) < (unsigned)W && (unsigned)(iy + j) < (unsigned)H) {
                            const size_t a = (size_t)(iy + j) * p.v.width + (size_t)(ix + i);
                            tg[2 * j + i] = p.pg[a];
                            th[2 * j + i] = p.ph[a];
                            tm[2 * j + i] = p.pm[a];
                        }
                    }
                }
            }
        }
    }
    vg_stage(p.v, sg, sl, tx0, ty0, tid);
    __syncthreads();
    if (!mine) return;
    const int cq = (ty + VR) * VW + tx + VR;
    const float l = sl[cq];
    // taps in the fixed order (0,0), (1,0), (0,1), (1,1); a tap outside the image holds Z' = 0
    const float b[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    float sb = 0.0f, h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, s1 = 0.0f, s2 = 0.0f, nmin = 255.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 g = tg[i];
        const bool ok = reproj && g.w > 0.0f && fabsf(g.w - zr) <= p.tau_z * zr &&
                        g.x * gp.x + g.y * gp.y + g.z * gp.z >= p.tau_n;
        const float bi = ok ? b[i] : 0.0f;
        sb += bi;
        h0 += bi * th[i].x;
        h1 += bi * th[i].y;
        h2 += bi * th[i].z;
        s1 += bi * tm[i].x;
        s2 += bi * tm[i].y;
        nmin = ok ? fminf(nmin, tm[i].z) : nmin;
    }
    float i0 = d0, i1 = d1, i2 = d2, m1 = l, m2 = l * l, n = 1.0f;
    if (sb >= 0.01f) {  // (sb > 0 needs a valid tap, so reproj holds and nmin is a tap's length)
        n = fminf(1.0f + nmin, 255.0f);
        const float alpha = fmaxf(p.alpha_min, 1.0f / n);
        h0 /= sb;
        h1 /= sb;
        h2 /= sb;
        s1 /= sb;
        s2 /= sb;
        i0 = h0 + alpha * (d0 - h0);
        i1 = h1 + alpha * (d1 - h1);
        i2 = h2 + alpha * (d2 - h2);
        m1 = s1 + alpha * (l - s1);
        m2 = s2 + alpha * (l * l - s2);
    }
    float var = fmaxf(0.0f, m2 - m1 * m1);
    if (__ballot(n < 4.0f) != 0ull) {  // wave-uniform
        const float var0 = vg_var0(p.v, sg, sl, cq, px, py);
        if (n < 4.0f) var = var0 / n;
    }
    p.v.rout[pix] = make_float4(i0, i1, i2, var);
    p.mout[pix] = make_float4(m1, m2, n, 0.0f);
    p.v.gout[pix] = gp;
}

// 3 x 3 inverse in f64 (columns a, b, c), row-major; false when the determinant is below 1e-12 of the
// product of the columns' lengths
bool invert3(const double* a, const double* b, const double* c, double inv[9]) {
    const double m[9] = {a[0], b[0], c[0], a[1], b[1], c[1], a[2], b[2], c[2]};
    const double co[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                          m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                          m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    const double det = m[0] * co[0] + m[1] * co[3] + m[2] * co[6];
    auto len = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const double scale = len(a) * len(b) * len(c);
    if (!(std::fabs(det) > 1e-12 * scale) || !std::isfinite(det)) return false;
    for (int i = 0; i < 9; ++i) inv[i] = co[i] / det;
    return true;
}

}  // namespace

// State (double-buffered by frame parity: a launch reads the previous records at gathered addresses
// while it writes the new ones) and work buffers, 16 B per pixel each: 2 guides, 2 moments, H, 2 work.
struct History {
    uint32_t width = 0, rows = 0;
    int device = -1;       // -1 until the first frame allocates
    uint32_t frames = 0;   // since new / reset
    uint32_t parity = 0;   // the buffers the last frame wrote
    bool written = false;  // a frame has ever been enqueued (read() has something to copy)
    TemporalCamera cam{};  // the last frame's
    float4* guides[2] = {nullptr, nullptr};
    float4* moments[2] = {nullptr, nullptr};
    float4* hist = nullptr;
    float4* work[2] = {nullptr, nullptr};
    float* io = nullptr;   // the host entry point's staging (11 f32 per pixel), on first use
};

History* gpu_history_new(uint32_t width, uint32_t rows) {
    auto* h = new History();
    h->width = width;
    h->rows = rows;
    return h;
}

void gpu_history_free(History* h) {
    if (!h) return;
    if (h->device >= 0) {
        int prev = 0;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(h->device);
        for (void* b : {(void*)h->guides[0], (void*)h->guides[1], (void*)h->moments[0], (void*)h->moments[1],
                        (void*)h->hist, (void*)h->work[0], (void*)h->work[1], (void*)h->io})
            (void)hipFree(b);
        (void)hipSetDevice(prev);
    }
    delete h;
}

void gpu_history_reset(History* h) { h->frames = 0; }
int gpu_history_device(const History* h) { return h->device; }

namespace {

void history_alloc(History* h, int device) {
    if (h->device >= 0) {
        if (h->device != device) throw std::invalid_argument("the history lives on another device");
        return;
    }
    const size_t bytes = (size_t)h->width * h->rows * sizeof(float4);
    float4* b[7] = {};
    for (auto& q : b) {
        if (hipMalloc((void**)&q, bytes) != hipSuccess) {
            for (auto& f : b) (void)hipFree(f);
            throw std::runtime_error("HIP error in hipMalloc(history): out of device memory");
        }
    }
    h->guides[0] = b[0], h->guides[1] = b[1], h->moments[0] = b[2], h->moments[1] = b[3];
    h->hist = b[4], h->work[0] = b[5], h->work[1] = b[6];
    h->device = device;
}

}  // namespace

float* gpu_history_io(History* h, int device) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    check(hipSetDevice(device), "hipSetDevice");
    hipError_t e = hipSuccess;
    try {
        history_alloc(h, device);
        if (!h->io) e = hipMalloc((void**)&h->io, (size_t)h->width * h->rows * 11 * sizeof(float));
    } catch (...) {
        (void)hipSetDevice(prev);
        throw;
    }
    (void)hipSetDevice(prev);
    check(e, "hipMalloc(history staging)");
    return h->io;
}

// temporal_kernel, then the K passes: pass 0 writes H (after the temporal kernel, the only reader of
// H', has finished: the same stream), the later passes ping-pong between the work buffers.
void gpu_denoise_temporal(History* h, int device, const TemporalCamera& cam, const float* colour, const float* albedo,
                          const float* normal, const float* depth, uint32_t iterations, float sigma_luminance,
                          float sigma_normal, float sigma_depth, float alpha_min, float tau_z, float tau_n, float* out,
                          float* out_variance, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    TemporalParams t{};
    const bool have_prev = h->frames > 0;
    double c[3], inv[9];
    for (int i = 0; i < 3; ++i) c[i] = cam.top_left[i] - cam.look_from[i];
    // (this camera is the next frame's M': rejected now, the history never holds a singular one)
    if (!invert3(cam.du, cam.dv, c, inv)) throw std::invalid_argument("denoise_temporal: the camera is singular");
    if (have_prev) {
        const TemporalCamera& o = h->cam;
        double co[3];
        for (int i = 0; i < 3; ++i) co[i] = o.top_left[i] - o.look_from[i];
        invert3(o.du, o.dv, co, inv);
        for (int r = 0; r < 3; ++r) {
            double tr = 0.0, e0 = 0.0, e1 = 0.0, e2 = 0.0;
            for (int i = 0; i < 3; ++i) {
                tr += inv[3 * r + i] * (cam.look_from[i] - o.look_from[i]);
                e0 += inv[3 * r + i] * (cam.du[i] - o.du[i]);
                e1 += inv[3 * r + i] * (cam.dv[i] - o.dv[i]);
                e2 += inv[3 * r + i] * (c[i] - co[i]);
            }
            t.t[r] = (float)tr;
            t.e[3 * r] = (float)e0, t.e[3 * r + 1] = (float)e1, t.e[3 * r + 2] = (float)e2;
        }
        for (int i = 0; i < 3; ++i) t.dl[i] = (float)(cam.look_from[i] - o.look_from[i]);
    }
    for (int i = 0; i < 3; ++i) {
        t.c0[i] = (float)(cam.top_left[i] - cam.look_from[i]);
        t.du[i] = (float)cam.du[i];
        t.dv[i] = (float)cam.dv[i];
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    check(hipSetDevice(device), "hipSetDevice");
    try {
        history_alloc(h, device);
    } catch (...) {
        (void)hipSetDevice(prev);
        throw;
    }
    const uint32_t cur = h->parity ^ 1u;
    t.v = vg_params(colour, albedo, normal, depth, h->width, h->rows, sigma_luminance, sigma_normal, sigma_depth, out,
                    out_variance);
    t.v.rout = h->work[0];
    t.v.gout = h->guides[cur];
    t.v.gin = h->guides[cur];
    t.pg = h->guides[h->parity];
    t.pm = h->moments[h->parity];
    t.ph = h->hist;
    t.mout = h->moments[cur];
    t.have_prev = have_prev ? 1u : 0u;
    t.alpha_min = alpha_min;
    t.tau_z = tau_z;
    t.tau_n = tau_n;
    hipLaunchKernelGGL(temporal_kernel, dim3((h->width + TW - 1) / TW, (h->rows + TH - 1) / TH), dim3(THREADS), 0,
                       stream, t);
    float4* const chain[6] = {h->work[0], h->hist, h->work[0], h->work[1], h->work[0], h->work[1]};
    enqueue_vg_passes(t.v, iterations, chain, stream);
    const hipError_t e = hipGetLastError();
    (void)hipSetDevice(prev);
    check(e, "denoise_temporal launch");
    h->parity = cur;
    h->cam = cam;
    h->frames += 1;
    h->written = true;
}

// (m1, m2) and n of the last frame, after everything enqueued on the history's device has finished
void gpu_history_read(History* h, float* moments, float* length) {
    if (!h->written) throw std::invalid_argument("history_read: no frame yet");
    const size_t n = (size_t)h->width * h->rows;
    std::vector<float4> rec(n);
    int prev = 0;
    (void)hipGetDevice(&prev);
    check(hipSetDevice(h->device), "hipSetDevice");
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(rec.data(), h->moments[h->parity], n * sizeof(float4), hipMemcpyDeviceToHost);
    (void)hipSetDevice(prev);
    check(e, "history_read");
    for (size_t i = 0; i < n; ++i) {
        if (moments) moments[2 * i] = rec[i].x, moments[2 * i + 1] = rec[i].y;
        if (length) length[i] = rec[i].z;
    }
}

}  // namespace nrt
