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
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "gpu.hpp"
#include "hip_util.hpp"

namespace nrt {

namespace {

constexpr int TW = 32, TH = 8;  // outputs per workgroup: one per lane, a wave = two rows of 32
constexpr int THREADS = TW * TH;
constexpr float ALBEDO_FLOOR = 1e-3f;

constexpr double LOG2E = 1.4426950408889634;

struct AtrousParams {
    const float* colour;  // FIRST: the caller's colour; else D_i (3 f32 per pixel)
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

// The fields the two filters' parameters share and every launch of a chain keeps (not gin, gout, pitch).  The
// structs keep their own layouts rather than embed a common one: the kernels' argument loads, and with them the
// generated code, stay what they were.
template <class P>
P frame_params(const float* colour, const float* albedo, const float* normal, const float* depth, uint32_t width,
               uint32_t rows, float sigma_normal, float sigma_depth, float* out) {
    P p{};
    p.colour = colour;
    p.albedo = albedo;
    p.normal = normal;
    p.depth = depth;
    p.cout = out;
    p.width = width;
    p.height = rows;
    p.kn = (float)(LOG2E / ((double)sigma_normal * sigma_normal));
    p.kz = (float)(LOG2E / ((double)sigma_depth * sigma_depth));
    return p;
}

// 0 <= v < n.  (The tests of x and of y stay two calls joined by && or || where they are used: joined inside a
// helper they compile to other code.)
__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// colour / max(albedo, floor) and its inverse, per channel value i
__device__ __forceinline__ float demodulate(const float* colour, const float* albedo, size_t i) {
    return colour[i] / fmaxf(albedo[i], ALBEDO_FLOOR);
}
__device__ __forceinline__ float remodulate(float d, const float* albedo, size_t i) {
    return d * fmaxf(albedo[i], ALBEDO_FLOOR);
}

// the guide record (normal.xyz, depth) of pixel a from the feature buffers
template <class P>
__device__ __forceinline__ float4 load_guide(const P& p, size_t a) {
    return make_float4(p.normal[3 * a], p.normal[3 * a + 1], p.normal[3 * a + 2], p.depth[a]);
}

// h = (1/16, 1/4, 3/8, 1/4, 1/16) and the 3 x 3 prefilter's (1/4, 1/2, 1/4)
__device__ __forceinline__ float h5(int i) {
    constexpr float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return hk[i];
}
__device__ __forceinline__ float g3(int i) {
    constexpr float gk[3] = {0.25f, 0.5f, 0.25f};
    return gk[i];
}

// The tile of one workgroup of a pass.  It computes TW x TH points of the lattice (x mod g, y mod g) = (lx, ly)
// and stages them plus a halo of 2 T points in LDS, T = s / g: with g = 1 that is an image-space tile
// with its 2 s halo (T = s = 1, 2, 4), with g = s the tile of an independent lattice of the
// step-s pass (T = 1), whose halo stays 2 points however large s is.  Region row-major, RW = TW + 4 T wide.
template <int T>
struct LatticeTile {
    static constexpr int RW = TW + 4 * T, RH = TH + 4 * T, NPIX = RW * RH;
    const uint32_t width;
    const int g, s, W, H, lx, ly, tx0, ty0;  // s = T g: the step; tx0, ty0: lattice coordinates
    template <class P>
    __device__ __forceinline__ explicit LatticeTile(const P& p)
        : width(p.width), g((int)p.pitch), s(T * g), W((int)p.width), H((int)p.height),
          lx((int)(blockIdx.x % p.pitch)), ly((int)(blockIdx.y % p.pitch)),
          tx0((int)(blockIdx.x / p.pitch) * TW), ty0((int)(blockIdx.y / p.pitch) * TH) {}
    // the tile's first pixel: (uniform) not in the image for a tile past the end of a short lattice
    __device__ __forceinline__ int x0() const { return lx + tx0 * g; }
    __device__ __forceinline__ int y0() const { return ly + ty0 * g; }
    // region slot q = v RW + u -> pixel (lx + (tx0 - 2 T + u) g, ly + (ty0 - 2 T + v) g), maybe outside the image
    __device__ __forceinline__ int2 slot_pixel(int q) const {
        const int v = q / RW, u = q - v * RW;
        return make_int2(lx + (tx0 - 2 * T + u) * g, ly + (ty0 - 2 * T + v) * g);
    }
    __device__ __forceinline__ size_t index(int2 xy) const { return (size_t)xy.y * width + (size_t)xy.x; }
    // A lane's own point (tx, ty), its pixel (px, py) and its region slot cq; tap (dx, dy) of the step: its slot,
    // and whether its row / column is in the image.
    struct Lane {
        const LatticeTile& t;
        const int tx, ty, px, py, cq;
        __device__ __forceinline__ Lane(const LatticeTile& tile, int tid)
            : t(tile), tx(tid % TW), ty(tid / TW), px(t.lx + (t.tx0 + tx) * t.g), py(t.ly + (t.ty0 + ty) * t.g),
              cq((ty + 2 * T) * RW + tx + 2 * T) {}
        __device__ __forceinline__ size_t pix() const { return (size_t)py * t.width + (size_t)px; }
        __device__ __forceinline__ int tap(int dx, int dy) const { return cq + dy * T * RW + dx * T; }
        __device__ __forceinline__ bool row_ok(int dy) const { return in_range(py + dy * t.s, t.H); }
        __device__ __forceinline__ bool col_ok(int dx) const { return in_range(px + dx * t.s, t.W); }
    };
};

// One pass over the packed colour.  LDS, over LatticeTile's region:
//   sc[3 (v RW + u) + c]  colour, packed as in memory: the staging loop's element e is written to
//                         word e (lane-contiguous, no conflict), and a tap read is word 3 u + const
//                         over the 32 lanes of a row: 3 is odd, so the 32 lanes hit 32 banks;
//   sg[v RW + u]          guide record, one 16-byte read per tap, lane-contiguous.
// Slots outside the image hold zeros and their taps get weight 0 from the coordinate test.
template <int T, bool FIRST, bool LAST>
__global__ void __launch_bounds__(THREADS) atrous_kernel(const AtrousParams p) {
    using Tile = LatticeTile<T>;
    __shared__ float4 sg[Tile::NPIX];
    __shared__ float sc[3 * Tile::NPIX];
    const Tile t(p);
    if (t.x0() >= t.W || t.y0() >= t.H) return;
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < 3 * Tile::NPIX; e += THREADS) {
        const int q = e / 3, c = e - 3 * q;
        const int2 xy = t.slot_pixel(q);
        float val = 0.0f;
        if (in_range(xy.x, t.W) && in_range(xy.y, t.H)) {
            const size_t a = t.index(xy) * 3u + (size_t)c;
            if constexpr (FIRST) val = demodulate(p.colour, p.albedo, a);
            else val = p.colour[a];
        }
        sc[e] = val;
    }
    for (int q = tid; q < Tile::NPIX; q += THREADS) {
        const int2 xy = t.slot_pixel(q);
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (in_range(xy.x, t.W) && in_range(xy.y, t.H)) {
            if constexpr (FIRST) r = load_guide(p, t.index(xy));
            else r = p.gin[t.index(xy)];
        }
        sg[q] = r;
    }
    __syncthreads();
    const typename Tile::Lane me(t, tid);
    if (me.px >= t.W || me.py >= t.H) return;
    const int cq = me.cq;
    const float4 gp = sg[cq];
    const float c0 = sc[3 * cq], c1 = sc[3 * cq + 1], c2 = sc[3 * cq + 2];
    float sw = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const bool oky = me.row_ok(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const bool ok = oky && me.col_ok(dx);
            const int q = me.tap(dx, dy);
            const float4 gq = sg[q];
            const float q0 = sc[3 * q], q1 = sc[3 * q + 1], q2 = sc[3 * q + 2];
            const float d0 = c0 - q0, d1 = c1 - q1, d2 = c2 - q2;
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
            const float e = (d0 * d0 + d1 * d1 + d2 * d2) * p.kc + (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
            // exp(-e) as one v_exp_f32 (the constants carry log2(e))
            const float w = ok ? h5(dx + 2) * h5(dy + 2) * __builtin_amdgcn_exp2f(-e) : 0.0f;
            sw += w;
            a0 += w * q0;
            a1 += w * q1;
            a2 += w * q2;
        }
    }
    // (the centre tap has e = 0: sw >= 9/64)
    float o0 = a0 / sw, o1 = a1 / sw, o2 = a2 / sw;
    const size_t pix = me.pix();
    if constexpr (LAST) {
        o0 = remodulate(o0, p.albedo, 3 * pix);
        o1 = remodulate(o1, p.albedo, 3 * pix + 1);
        o2 = remodulate(o2, p.albedo, 3 * pix + 2);
    }
    p.cout[3 * pix] = o0;
    p.cout[3 * pix + 1] = o1;
    p.cout[3 * pix + 2] = o2;
    if constexpr (FIRST) {
        if (p.gout) p.gout[pix] = gp;
    }
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

// Pass i of a frame: step 2^i on tiles of pitch g (lattice_from()), taps T = step / g points apart; the grid has
// the lattice (lx, ly) in the low part of the block index: neighbouring workgroups read the same lines.
struct Pass {
    uint32_t step, pitch, T;
    dim3 grid;
};
Pass pass_of(uint32_t i, uint32_t width, uint32_t rows, uint32_t lat) {
    const uint32_t step = 1u << i, g = step >= lat ? step : 1u;
    const uint32_t lw = (width + g - 1) / g, lh = (rows + g - 1) / g;
    return {step, g, step / g, dim3(((lw + TW - 1) / TW) * g, ((lh + TH - 1) / TH) * g)};
}

// f(std::integral_constant<int, T>) for T = 1, 2, 4: the pass kernels' template argument
template <class F>
void with_T(uint32_t t, F&& f) {
    if (t == 1) f(std::integral_constant<int, 1>());
    else if (t == 2) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 4>());
}

// (destructors: no exception leaves; a device that cannot be made current has nothing left to free)
void free_on_device(int device, std::initializer_list<void*> ptrs) noexcept {
    try {
        DeviceGuard guard(device);
        for (void* p : ptrs) (void)hipFree(p);
    } catch (...) {
    }
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
    free_on_device(s->device, {s->ping, s->pong, s->guides});
    delete s;
}

DenoiseScratch* gpu_denoise_scratch(DenoiseScratch* have, size_t pixels, int device, size_t rec_bytes) {
    if (have && have->device == device && have->pixels >= pixels && have->rec_bytes >= rec_bytes) return have;
    gpu_denoise_scratch_free(have);  // (hipFree waits for the device: no pass still reads the old buffers)
    std::unique_ptr<DenoiseScratch, decltype(&gpu_denoise_scratch_free)> s(new DenoiseScratch(), gpu_denoise_scratch_free);
    s->device = device;
    DeviceGuard guard(device);
    check(hipMalloc((void**)&s->ping, pixels * rec_bytes), "hipMalloc(denoise scratch)");
    check(hipMalloc((void**)&s->pong, pixels * rec_bytes), "hipMalloc(denoise scratch)");
    check(hipMalloc((void**)&s->guides, pixels * sizeof(float4)), "hipMalloc(denoise scratch)");
    s->pixels = pixels;
    s->rec_bytes = rec_bytes;
    return s.release();
}

void gpu_denoise(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                 uint32_t width, uint32_t rows, uint32_t iterations, float sigma_color, float sigma_normal,
                 float sigma_depth, float* out, void* stream_ptr) {
    const size_t pixels = (size_t)width * rows;
    if (!s || s->pixels < pixels || s->rec_bytes < 3 * sizeof(float)) throw std::runtime_error("denoise scratch too small");
    hipStream_t stream = (hipStream_t)stream_ptr;
    DeviceGuard guard(s->device);
    const uint32_t lat = lattice_from();
    // a single pass in place would read the halo of pixels other workgroups have already replaced
    const bool alias = iterations == 1 && colour < out + pixels * 3 && out < colour + pixels * 3;
    auto p = frame_params<AtrousParams>(colour, albedo, normal, depth, width, rows, sigma_normal, sigma_depth, nullptr);
    p.gin = s->guides;
    float* bufs[2] = {s->ping, s->pong};
    for (uint32_t i = 0; i < iterations; ++i) {
        const bool first = i == 0, last = i + 1 == iterations;
        const Pass pass = pass_of(i, width, rows, lat);
        p.gout = last ? nullptr : s->guides;
        p.cout = last && !alias ? out : bufs[i & 1u];
        p.pitch = pass.pitch;
        const double sc = (double)sigma_color / (double)pass.step;
        p.kc = (float)(LOG2E / (sc * sc));
        with_T(pass.T, [&](auto T) { launch_pass<decltype(T)::value>(p, first, last, pass.grid, stream); });
        p.colour = p.cout;
    }
    check(hipGetLastError(), "denoise launch");
    if (alias) check(hipMemcpyAsync(out, p.colour, pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream), "denoise launch");
}

// ---- variance-guided filter: 7 x 7 moments kernel, then K passes over (colour, variance) records
namespace {

constexpr int VR = 3;                                   // the moments window's radius
constexpr int VW = TW + 2 * VR, VH = TH + 2 * VR;       // 38 x 14 slots
constexpr int VPIX = VW * VH;

__device__ __forceinline__ float lum(float r, float g, float b) {
    return fmaf(0.2126f, r, fmaf(0.7152f, g, 0.0722f * b));
}

// Var_0 and the records of the passes.  A workgroup computes 32 x 8 pixels and stages them plus a halo
// of 3 in LDS, 38 x 14 slots: one word of demodulated luminance and one 16-byte guide record each
// (4 B + 16 B, 10.6 KB).  Consecutive lanes read consecutive words / records at every tap, so neither
// array has a bank conflict.  Each lane sums its 49 taps in one fixed order; the luminance is shifted
// by the centre's, so the two moments stay of the noise's size and their difference does not cancel.
// (The two halves below are shared with temporal_kernel; the staging loop, with another word per slot, with
// vg_dual_kernel.)
// Stage the region's guide records and one word per slot, word(a) of pixel a; slots outside the image hold zeros.
template <class F>
__device__ __forceinline__ void vg_stage_words(const VgParams& p, float4* sg, float* sl, int tx0, int ty0, int tid,
                                               F&& word) {
    const int W = (int)p.width, H = (int)p.height;
    for (int q = tid; q < VPIX; q += THREADS) {
        const int v = q / VW, u = q - v * VW;
        const int x = tx0 - VR + u, y = ty0 - VR + v;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float l = 0.0f;
        if (in_range(x, W) && in_range(y, H)) {
            const size_t a = (size_t)y * p.width + (size_t)x;
            r = load_guide(p, a);
            l = word(a);
        }
        sg[q] = r;
        sl[q] = l;
    }
}

// the word of the moments and the temporal kernel: the demodulated luminance
__device__ __forceinline__ void vg_stage(const VgParams& p, float4* sg, float* sl, int tx0, int ty0, int tid) {
    vg_stage_words(p, sg, sl, tx0, ty0, tid, [&](size_t a) {
        return lum(demodulate(p.colour, p.albedo, 3 * a), demodulate(p.colour, p.albedo, 3 * a + 1),
                   demodulate(p.colour, p.albedo, 3 * a + 2));
    });
}

// Var_0 of the pixel (px, py) at region slot cq
__device__ __forceinline__ float vg_var0(const VgParams& p, const float4* sg, const float* sl, int cq, int px, int py) {
    const int W = (int)p.width, H = (int)p.height;
    const float4 gp = sg[cq];
    const float lp = sl[cq];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
    for (int dy = -VR; dy <= VR; ++dy) {
        const bool oky = in_range(py + dy, H);
#pragma unroll
        for (int dx = -VR; dx <= VR; ++dx) {
            const bool ok = oky && in_range(px + dx, W);
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
    p.rout[pix] = make_float4(demodulate(p.colour, p.albedo, 3 * pix), demodulate(p.colour, p.albedo, 3 * pix + 1),
                              demodulate(p.colour, p.albedo, 3 * pix + 2), var0);
    p.gout[pix] = sg[cq];
}

// ---- dual-buffer variance: Var_0 from two frames A, B of one camera over disjoint sample windows of equal
//      length (formula: nrt.h, nrt_denoise_vg_dual).  The moments kernel's place in the chain and its contract:
//      it writes (D_0.rgb, Var_0) and the packed guide record of every pixel, and the passes follow unchanged.
struct VgDualParams {
    VgParams v;           // colour = A, albedo, normal, depth, width, height, kn, kz, rout, gout
    const float* colour_b;
};

// (A[i] + B[i]) / 2 over max(albedo, floor), and the half difference's channel before the luminance
__device__ __forceinline__ float dual_mean(const VgDualParams& p, size_t i) {
    return ((p.v.colour[i] + p.colour_b[i]) * 0.5f) / fmaxf(p.v.albedo[i], ALBEDO_FLOOR);
}
__device__ __forceinline__ float dual_diff(const VgDualParams& p, size_t i) {
    return (p.v.colour[i] - p.colour_b[i]) / fmaxf(p.v.albedo[i], ALBEDO_FLOOR);
}

// The moments kernel's tile, staging and LDS layout (32 x 8 outputs, halo 3, 38 x 14 slots of one word and one
// 16-byte guide record, 10 640 B; consecutive lanes read consecutive words / records at every tap: no bank
// conflict), with another word: delta^2, delta = lum((A - B) / a) / 2, three divisions per slot, both colour
// buffers and the albedo read once per slot.  E[delta^2] is the variance of lum(D_0) for independent halves, so
// the word is a one-sample estimate of the noise alone and the 49 guide-weighted taps pool it: one weighted sum
// (no first moment to subtract, no shift by the centre), and no luminance in the weight, since an edge of the
// image is no evidence of noise.  Each lane sums its taps in one fixed order, rows not unrolled, the 7 taps of a
// row unrolled; no atomics, plain vector stores.  A == B gives delta = 0 in every slot and Var_0 = 0 exactly.
__global__ void __launch_bounds__(THREADS) vg_dual_kernel(const VgDualParams p) {
    __shared__ float4 sg[VPIX];
    __shared__ float sd[VPIX];
    const VgParams& f = p.v;
    const int W = (int)f.width, H = (int)f.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
    vg_stage_words(f, sg, sd, tx0, ty0, tid, [&](size_t a) {
        const float d = 0.5f * lum(dual_diff(p, 3 * a), dual_diff(p, 3 * a + 1), dual_diff(p, 3 * a + 2));
        return d * d;
    });
    __syncthreads();
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    if (px >= W || py >= H) return;
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
            const float e = (n0 * n0 + n1 * n1 + n2 * n2) * f.kn + dz * dz * f.kz;
            const float w = ok ? __builtin_amdgcn_exp2f(-e) : 0.0f;
            sw += w;
            s2 += w * sd[q];
        }
    }
    // (the centre tap has w = 1: sw >= 1)
    const size_t pix = (size_t)py * f.width + (size_t)px;
    // the lane's own D_0 from memory: the lines the staging loop just read
    f.rout[pix] = make_float4(dual_mean(p, 3 * pix), dual_mean(p, 3 * pix + 1), dual_mean(p, 3 * pix + 2), s2 / sw);
    f.gout[pix] = gp;
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
    using Tile = LatticeTile<T>;
    __shared__ float4 sr[Tile::NPIX];
    __shared__ float4 sg[Tile::NPIX];
    const Tile t(p);
    if (t.x0() >= t.W || t.y0() >= t.H) return;
    const int tid = (int)threadIdx.x;
    const typename Tile::Lane me(t, tid);
    const bool mine = me.px < t.W && me.py < t.H;
    float pv = 0.0f, pk = 0.0f;
    if (mine) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = me.px + dx, y = me.py + dy;
                if (in_range(x, t.W) && in_range(y, t.H)) {
                    pv += g3(dx + 1) * g3(dy + 1) * p.rin[(size_t)y * p.width + (size_t)x].w;
                    pk += g3(dx + 1) * g3(dy + 1);
                }
            }
        }
    }
    for (int q = tid; q < Tile::NPIX; q += THREADS) {
        const int2 xy = t.slot_pixel(q);
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f), k = r;
        if (in_range(xy.x, t.W) && in_range(xy.y, t.H)) {
            r = p.rin[t.index(xy)];
            k = p.gin[t.index(xy)];
        }
        sr[q] = r;
        sg[q] = k;
    }
    __syncthreads();
    if (!mine) return;
    const int cq = me.cq;
    const float4 gp = sg[cq], rp = sr[cq];
    const float lp = lum(rp.x, rp.y, rp.z);
    // log2(e) / (sigma_l sigma(p) + 1e-6): the centre tap's own weight 1/4 keeps pk >= 1/4
    const float kl = (float)LOG2E / (p.sigma_l * sqrtf(pv / pk) + 1e-6f);
    float sw = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, av = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const bool oky = me.row_ok(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const bool ok = oky && me.col_ok(dx);
            const int q = me.tap(dx, dy);
            const float4 gq = sg[q], rq = sr[q];
            const float dl = fabsf(lp - lum(rq.x, rq.y, rq.z));
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z, dz = gp.w - gq.w;
            const float e = dl * kl + (n0 * n0 + n1 * n1 + n2 * n2) * p.kn + dz * dz * p.kz;
            const float w = ok ? h5(dx + 2) * h5(dy + 2) * __builtin_amdgcn_exp2f(-e) : 0.0f;
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
    const size_t pix = me.pix();
    if constexpr (LAST) {
        p.cout[3 * pix] = remodulate(o0, p.albedo, 3 * pix);
        p.cout[3 * pix + 1] = remodulate(o1, p.albedo, 3 * pix + 1);
        p.cout[3 * pix + 2] = remodulate(o2, p.albedo, 3 * pix + 2);
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
        const Pass pass = pass_of(i, p.width, p.height, lat);
        p.rin = chain[i];
        p.rout = chain[i + 1];
        p.pitch = pass.pitch;
        with_T(pass.T, [&](auto T) { launch_vg_pass<decltype(T)::value>(p, i + 1 == iterations, pass.grid, stream); });
    }
}

// The chain of the two single-frame entry points on the scratch: first(p, grid, stream) launches the kernel that
// writes (D_0, Var_0) and the guide records, then the K passes ping-pong.
template <class F>
void vg_chain(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
              uint32_t width, uint32_t rows, uint32_t iterations, float sigma_luminance, float sigma_normal,
              float sigma_depth, float* out, float* out_variance, void* stream_ptr, const char* what, F&& first) {
    const size_t pixels = (size_t)width * rows;
    if (!s || s->pixels < pixels || s->rec_bytes < sizeof(float4)) throw std::runtime_error("denoise scratch too small");
    hipStream_t stream = (hipStream_t)stream_ptr;
    DeviceGuard guard(s->device);
    float4* const b0 = (float4*)s->ping;
    float4* const b1 = (float4*)s->pong;
    float4* const chain[6] = {b0, b1, b0, b1, b0, b1};
    auto p = frame_params<VgParams>(colour, albedo, normal, depth, width, rows, sigma_normal, sigma_depth, out);
    p.vout = out_variance;
    p.sigma_l = sigma_luminance;
    p.rout = b0;
    p.gin = s->guides;
    p.gout = s->guides;
    first(p, dim3((width + TW - 1) / TW, (rows + TH - 1) / TH), stream);
    enqueue_vg_passes(p, iterations, chain, stream);
    check(hipGetLastError(), what);
}

}  // namespace

// The moments kernel reads the caller's colour and no pass does (the last one reads the albedo), so
// out == colour needs no copy for any K.
void gpu_denoise_vg(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                    uint32_t width, uint32_t rows, uint32_t iterations, float sigma_luminance, float sigma_normal,
                    float sigma_depth, float* out, float* out_variance, void* stream_ptr) {
    vg_chain(s, colour, albedo, normal, depth, width, rows, iterations, sigma_luminance, sigma_normal, sigma_depth, out,
             out_variance, stream_ptr, "denoise_vg launch", [](const VgParams& p, dim3 grid, hipStream_t stream) {
                 hipLaunchKernelGGL(vg_moments_kernel, grid, dim3(THREADS), 0, stream, p);
             });
}

// Likewise the dual kernel is the only reader of the two colour buffers: out may be either, for any K.
void gpu_denoise_vg_dual(DenoiseScratch* s, const float* colour_a, const float* colour_b, const float* albedo,
                         const float* normal, const float* depth, uint32_t width, uint32_t rows, uint32_t iterations,
                         float sigma_luminance, float sigma_normal, float sigma_depth, float* out, float* out_variance,
                         void* stream_ptr) {
    vg_chain(s, colour_a, albedo, normal, depth, width, rows, iterations, sigma_luminance, sigma_normal, sigma_depth,
             out, out_variance, stream_ptr, "denoise_vg_dual launch",
             [colour_b](const VgParams& p, dim3 grid, hipStream_t stream) {
                 hipLaunchKernelGGL(vg_dual_kernel, grid, dim3(THREADS), 0, stream, VgDualParams{p, colour_b});
             });
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
    const VgParams& f = p.v;
    const int W = (int)f.width, H = (int)f.height;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const int tid = (int)threadIdx.x;
    const int tx = tid % TW, ty = tid / TW;
    const int px = tx0 + tx, py = ty0 + ty;
    const bool mine = px < W && py < H;
    const size_t pix = mine ? (size_t)py * f.width + (size_t)px : 0;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 tg[4] = {zero, zero, zero, zero}, th[4] = {zero, zero, zero, zero}, tm[4] = {zero, zero, zero, zero};
    float4 gp = zero;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, fx = 0.0f, fy = 0.0f, zr = 0.0f;
    bool reproj = false;
    if (mine) {
        gp = load_guide(f, pix);
        d0 = demodulate(f.colour, f.albedo, 3 * pix);
        d1 = demodulate(f.colour, f.albedo, 3 * pix + 1);
        d2 = demodulate(f.colour, f.albedo, 3 * pix + 2);
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
                        if (in_range(ix + i, W) && in_range(iy + j, H)) {
                            const size_t a = (size_t)(iy + j) * f.width + (size_t)(ix + i);
                            tg[2 * j + i] = p.pg[a];
                            th[2 * j + i] = p.ph[a];
                            tm[2 * j + i] = p.pm[a];
                        }
                    }
                }
            }
        }
    }
    vg_stage(f, sg, sl, tx0, ty0, tid);
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
        const float var0 = vg_var0(f, sg, sl, cq, px, py);
        if (n < 4.0f) var = var0 / n;
    }
    p.v.rout[pix] = make_float4(i0, i1, i2, var);
    p.mout[pix] = make_float4(m1, m2, n, 0.0f);
    f.gout[pix] = gp;
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
    if (h->device >= 0)
        free_on_device(h->device, {h->guides[0], h->guides[1], h->moments[0], h->moments[1], h->hist, h->work[0],
                                   h->work[1], h->io});
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
    DeviceGuard guard(device);
    history_alloc(h, device);
    if (!h->io) check(hipMalloc((void**)&h->io, (size_t)h->width * h->rows * 11 * sizeof(float)), "hipMalloc(history staging)");
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
    DeviceGuard guard(device);
    history_alloc(h, device);
    const uint32_t cur = h->parity ^ 1u;
    t.v = frame_params<VgParams>(colour, albedo, normal, depth, h->width, h->rows, sigma_normal, sigma_depth, out);
    t.v.vout = out_variance;
    t.v.sigma_l = sigma_luminance;
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
    check(hipGetLastError(), "denoise_temporal launch");
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
    DeviceGuard guard(h->device);
    check(hipDeviceSynchronize(), "history_read");
    check(hipMemcpy(rec.data(), h->moments[h->parity], n * sizeof(float4), hipMemcpyDeviceToHost), "history_read");
    for (size_t i = 0; i < n; ++i) {
        if (moments) moments[2 * i] = rec[i].x, moments[2 * i + 1] = rec[i].y;
        if (length) length[i] = rec[i].z;
    }
}

}  // namespace nrt
