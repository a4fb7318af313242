// Feature buffers of the first hit (albedo, shading normal, depth) for the edge-avoiding filter
// (denoise.hip): one un-jittered primary ray per pixel through the f32 kernels' own trace<>,
// make_record<> and tex_color<>.  No reference counterpart (the reference writes the frame only).
// Built with the fast kernels' contraction flag.
#include "kernel.hpp"
#include "launch.hpp"

namespace nrt {

namespace dev {

// One pixel per lane.  The primary ray is Camera::get_ray without its draws (camera.rs:244-267 at
// spp = 1, no defocus, time 0): origin look_from, direction top_left + x du + y dv - look_from.
// MAXD as render_kernel's: 0 world list, -1 world BVH, 1 / MAX_INSTANCE_DEPTH the instance BVH.
// The scene tables stay in global memory: a lane makes one query, so a workgroup would copy the
// scene into LDS for 256 rays (the render's persistent waves amortise that copy over thousands);
// the world list's records arrive through the scalar cache either way.  Dynamic LDS holds only the
// world-BVH stack, tree bound + 1 entries per lane, BLOCK apart (launch_impl.hpp launch_one).
template <int MAXD, int KFLAGS>
__global__ void __launch_bounds__(BLOCK) aov_kernel(const RenderParams p, const DSceneView<float> sc,
                                                     float* __restrict__ albedo, float* __restrict__ normal,
                                                     float* __restrict__ depth) {
    using R = float;
    constexpr bool PERLIN = (KFLAGS & KF_PERLIN) != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int32_t* const stack = MAXD < 0 ? (int32_t*)lds + threadIdx.x : nullptr;
    const uint32_t i = p.pixel_begin + blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.pixel_end) return;  // (no barrier follows)
    const uint32_t x = i % p.width, y = p.row_offset + (i / p.width) * p.row_stride;
    auto cam = [&](int q) { return mk(p.camf[q][0], p.camf[q][1], p.camf[q][2]); };
    Ray<R> ray;
    ray.o = cam(3);
    ray.d = vfma((R)y, cam(2), vfma((R)x, cam(1), cam(0))) - ray.o;
    ray.time = R(0);
    prep_ray<R, false>(ray);
    HitMin<R, MAXD> hm;
    const bool hit = trace<R, MAXD, false, false, false, NoSig>(sc, ray, hm, stack);
    V<R> a = cam(6), n = mk(R(0), R(0), R(0));  // miss: the background, no normal, depth 0
    R z = R(0);
    if (hit) {
        const Rec<R> h = make_record<R, MAXD, false, false, false, false>(sc, ray, hm);
        const DMatFast m = sc.mats_fast[h.mat];
        if (m.kind == MAT_DIELECTRIC) {
            a = mk(R(1), R(1), R(1));
        } else if (m.solid) {
            a = mk(m.color[0], m.color[1], m.color[2]);
        } else {  // the texture's colour; a light's is not scaled by its intensity
            R u = h.u, v = h.v;
            if (MAXD <= 0 && u == R(UV_DEFERRED)) sphere_uv(h, u, v);
            a = tex_color<R, PERLIN>(sc, m.texture, u, v, h.p);
        }
        n = h.n;
        const V<R> dp = h.p - ray.o;
        z = sqrtf(dot(dp, dp));
    }
    if (albedo) {
        albedo[3ull * i] = a.x;
        albedo[3ull * i + 1] = a.y;
        albedo[3ull * i + 2] = a.z;
    }
    if (normal) {
        normal[3ull * i] = n.x;
        normal[3ull * i + 1] = n.y;
        normal[3ull * i + 2] = n.z;
    }
    if (depth) depth[i] = z;
}

}  // namespace dev

template <int MAXD>
static void launch_aov_mode(const RenderParams& p, const DSceneView<float>& v, bool perlin, float* albedo,
                            float* normal, float* depth, hipStream_t stream) {
    const uint32_t npix = p.pixel_end - p.pixel_begin;
    const uint32_t blocks = (npix + dev::BLOCK - 1) / dev::BLOCK;
    const uint32_t lds = MAXD < 0 ? (v.wbvh_stack + 1u) * dev::BLOCK * (uint32_t)sizeof(int32_t) : 0u;
    if (perlin)
        hipLaunchKernelGGL((dev::aov_kernel<MAXD, dev::KF_PERLIN>), dim3(blocks), dim3(dev::BLOCK), lds, stream, p, v,
                           albedo, normal, depth);
    else
        hipLaunchKernelGGL((dev::aov_kernel<MAXD, 0>), dim3(blocks), dim3(dev::BLOCK), lds, stream, p, v, albedo,
                           normal, depth);
}

void launch_aov(const RenderParams& p, const DSceneView<float>& v, int maxd, bool perlin, float* albedo, float* normal,
                float* depth, hipStream_t stream) {
    if (maxd == MODE_WORLD_BVH) launch_aov_mode<MODE_WORLD_BVH>(p, v, perlin, albedo, normal, depth, stream);
    else if (maxd == MODE_WORLD_LIST) launch_aov_mode<MODE_WORLD_LIST>(p, v, perlin, albedo, normal, depth, stream);
    else if (maxd == 1) launch_aov_mode<1>(p, v, perlin, albedo, normal, depth, stream);
    else launch_aov_mode<MAX_INSTANCE_DEPTH>(p, v, perlin, albedo, normal, depth, stream);
}

}  // namespace nrt
