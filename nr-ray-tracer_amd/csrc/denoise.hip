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
__global__ void __launch_bounds__(THREADS) vg_moments_kernel(const VgParams p) {
    __shared__ float4 sg[VPIX];
    __shared__ float sl[VPIX];
    const int W = (int)p.width, H = (int)p.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
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
    __syncthreads();
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    if (px >= W || py >= H) return;
    const int cq = (ty + VR) * VW + tx + VR;
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
    const size_t pix = (size_t)py * p.width + (size_t)px;
    // the lane's own D_0 again from memory (the lines the staging loop just read): the same divisions,
    // so the luminance of this record is the staged one
    p.rout[pix] = make_float4(p.colour[3 * pix] / fmaxf(p.albedo[3 * pix], ALBEDO_FLOOR),
                              p.colour[3 * pix + 1] / fmaxf(p.albedo[3 * pix + 1], ALBEDO_FLOOR),
                              p.colour[3 * pix + 2] / fmaxf(p.albedo[3 * pix + 2], ALBEDO_FLOOR),
                              fmaxf(0.0f, m2 - m1 * m1));
    p.gout[pix] = gp;
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
    const double log2e = 1.4426950408889634;
    const uint32_t lat = lattice_from();
    float4* bufs[2] = {(float4*)s->ping, (float4*)s->pong};
    VgParams p{};
    p.colour = colour;
    p.albedo = albedo;
    p.normal = normal;
    p.depth = depth;
    p.gin = s->guides;
    p.gout = s->guides;
    p.cout = out;
    p.vout = out_variance;
    p.width = width;
    p.height = rows;
    p.sigma_l = sigma_luminance;
    p.kn = (float)(log2e / ((double)sigma_normal * sigma_normal));
    p.kz = (float)(log2e / ((double)sigma_depth * sigma_depth));
    p.rout = bufs[0];
    hipLaunchKernelGGL(vg_moments_kernel, dim3((width + TW - 1) / TW, (rows + TH - 1) / TH), dim3(THREADS), 0, stream, p);
    for (uint32_t i = 0; i < iterations; ++i) {
        const uint32_t step = 1u << i, g = step >= lat ? step : 1u;
        p.rin = bufs[i & 1u];
        p.rout = bufs[(i + 1u) & 1u];
        p.pitch = g;
        const uint32_t lw = (width + g - 1) / g, lh = (rows + g - 1) / g;
        const dim3 grid(((lw + TW - 1) / TW) * g, ((lh + TH - 1) / TH) * g);
        if (step / g == 1) launch_vg_pass<1>(p, i + 1 == iterations, grid, stream);
        else if (step / g == 2) launch_vg_pass<2>(p, i + 1 == iterations, grid, stream);
        else launch_vg_pass<4>(p, i + 1 == iterations, grid, stream);
    }
    const hipError_t e = hipGetLastError();
    (void)hipSetDevice(prev);
    check(e, "denoise_vg launch");
}

}  // namespace nrt
