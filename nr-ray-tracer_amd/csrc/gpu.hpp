// Host-side interface to the HIP layer (render.hip).  Plain C++ types only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "render_params.hpp"

namespace nrt {

struct FlatScene;
struct DeviceScene;
struct MultiRender;

// Multi-GPU render in one process (multi.hip): scenes[d] on device first + d (consecutive), one
// RCCL communicator per device (ncclCommInitAll), rows y = d (mod N) on device d, one ncclGather
// to the first device and a row un-permute there.  p is the full-frame RenderParams.  loopback
// (tests): every scenes[d] is on the first device and the gather is device-to-device copies.
MultiRender* gpu_multi_create(const std::vector<DeviceScene*>& scenes, bool loopback);  // throws
bool gpu_multi_rccl_usable(std::string* why);
void gpu_multi_prepare(MultiRender* m, uint32_t width, uint32_t height);  // shard / staging buffers now  // librccl loadable with ncclGather / ncclCommInitAll
void gpu_multi_free(MultiRender* m);
int gpu_multi_first(const MultiRender* m);
int gpu_multi_count(const MultiRender* m);
// asynchronous: dev_out (first device) is written after `stream`'s prior work, and `stream` waits for it
void gpu_multi_render_device(MultiRender* m, const RenderParams& p, uint32_t precision, uint32_t rng, uint32_t trace,
                             float* dev_out, void* stream);
// synchronous: the frame lands in host memory
void gpu_multi_render_host(MultiRender* m, const RenderParams& p, uint32_t precision, uint32_t rng, uint32_t trace,
                           float* host_out);
// HIP-event times (ms) of the last frame: out[d] = device first + d's render kernel, out[N] = the
// gather + un-permute on the first device, out[N + 1] = the device time per frame since the previous
// call: the first device's render start of the window's first frame to the last frame's completion,
// over the frames (0 with fewer than two); a call that writes out[N + 1] starts a new window; returns N + 2
size_t gpu_multi_timings(MultiRender* m, float* out, size_t n);

int gpu_device_count();
DeviceScene* gpu_upload_scene(const FlatScene& fs, int device);  // throws std::runtime_error
void gpu_free_scene(DeviceScene* ds);
size_t gpu_scene_bytes(const DeviceScene* ds);
int gpu_scene_device(const DeviceScene* ds);
// Enqueue one render launch on `stream` (nullptr = default stream). p.out is a device pointer.
void gpu_launch_render(const DeviceScene* ds, const RenderParams& p, uint32_t precision, uint32_t rng, uint32_t trace,
                       void* stream);
// f32 kernel mode for nrt_trace `trace`: 0 = world-space list, 1 / MAX_INSTANCE_DEPTH = instance BVH.
int gpu_fast_maxd(const DeviceScene* ds, uint32_t trace);
// Enqueue the feature-buffer pass (aov.hip) on `stream`: first-hit albedo / normal (3 f32 per pixel) and
// depth (1 f32) of the rows p selects, device pointers, any of them null; traversal as the f32 render's.
void gpu_launch_aov(const DeviceScene* ds, const RenderParams& p, uint32_t trace, float* albedo, float* normal,
                    float* depth, void* stream);
// A-trous filter (denoise.hip).  The scratch (two colour buffers and the packed guide records) holds
// `pixels` pixels on `device`; gpu_denoise_scratch returns `have` when it is large enough, else frees it
// and allocates anew (have may be null).  rec_bytes: a colour buffer's bytes per pixel, 12 for gpu_denoise,
// 16 (colour and variance) for gpu_denoise_vg.
struct DenoiseScratch;
DenoiseScratch* gpu_denoise_scratch(DenoiseScratch* have, size_t pixels, int device, size_t rec_bytes = 12);  // throws
void gpu_denoise_scratch_free(DenoiseScratch* s);
// Enqueue the `iterations` passes on `stream` (device pointers; out may be colour); sigmas > 0.
void gpu_denoise(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                 uint32_t width, uint32_t rows, uint32_t iterations, float sigma_color, float sigma_normal,
                 float sigma_depth, float* out, void* stream);
// Variance-guided filter: the moments kernel and the `iterations` passes (scratch with rec_bytes 16; out may
// be colour; out_variance may be null).
void gpu_denoise_vg(DenoiseScratch* s, const float* colour, const float* albedo, const float* normal, const float* depth,
                    uint32_t width, uint32_t rows, uint32_t iterations, float sigma_luminance, float sigma_normal,
                    float sigma_depth, float* out, float* out_variance, void* stream);
// The same chain with the variance taken from two frames of one camera over disjoint sample windows (vg_dual_kernel in
// the moments kernel's place); out may be either colour buffer.
void gpu_denoise_vg_dual(DenoiseScratch* s, const float* colour_a, const float* colour_b, const float* albedo,
                         const float* normal, const float* depth, uint32_t width, uint32_t rows, uint32_t iterations,
                         float sigma_luminance, float sigma_normal, float sigma_depth, float* out, float* out_variance,
                         void* stream);
// Temporal accumulation in front of the variance-guided passes (denoise.hip).  A History holds the
// previous frame's camera, guide records, colour history, luminance moments and history length for
// width x rows pixels, plus the work buffers of the passes: 112 B per pixel, allocated on `device`
// by the first frame (gpu_history_io: now, plus the host entry point's staging of colour | albedo |
// normal | depth | variance, 11 f32 per pixel).
struct TemporalCamera {
    double look_from[3], du[3], dv[3], top_left[3];
};
struct History;
History* gpu_history_new(uint32_t width, uint32_t rows);
void gpu_history_free(History* h);
void gpu_history_reset(History* h);       // the next frame's history is invalid everywhere
int gpu_history_device(const History* h);  // -1: nothing allocated yet
float* gpu_history_io(History* h, int device);  // throws
// Enqueue the temporal kernel and the `iterations` (2..5) passes on `stream`; out may be colour,
// out_variance may be null.  std::invalid_argument for a singular camera or another device than the first frame's.
void gpu_denoise_temporal(History* h, int device, const TemporalCamera& cam, const float* colour, const float* albedo,
                          const float* normal, const float* depth, uint32_t iterations, float sigma_luminance,
                          float sigma_normal, float sigma_depth, float alpha_min, float tau_z, float tau_n, float* out,
                          float* out_variance, void* stream);
// Waits for the device, then copies out the last frame's (m1, m2) (2 f32 per pixel) and n (1 f32); either may be null.
void gpu_history_read(History* h, float* moments, float* length);
// Adaptive sampling (adaptive.hip).  The scratch holds, for `pixels` pixels on `device`: the half means A, B and the
// samples per half n, the pixel list, the list render's compact A', B', the feature buffers, and the select chain's
// tile masks, counts and offsets (84 B per pixel and 40 B per tile); gpu_adaptive_scratch follows gpu_denoise_scratch.
struct AdaptiveScratch;
struct AdaptiveBuffers {
    float *a, *b;          // 3 f32 per pixel
    uint32_t* n;           // 1 per pixel
    uint32_t* list;        // up to `pixels` entries
    float *a_new, *b_new;  // 3 f32 per list entry
    float *albedo, *normal, *depth;
};
AdaptiveScratch* gpu_adaptive_scratch(AdaptiveScratch* have, size_t pixels, int device);  // throws
void gpu_adaptive_scratch_free(AdaptiveScratch* s);
AdaptiveBuffers gpu_adaptive_buffers(const AdaptiveScratch* s);
// Enqueue select, scan and scatter on `stream` (device pointers; the scratch's masks, counts and offsets): the pixels
// with n == level and err >= threshold into `list` in tile order (at most `cap` entries written), their number into
// *total (null: the scratch's own word, which gpu_adaptive_count reads), err (may be null) for every pixel.
void gpu_adaptive_select(AdaptiveScratch* s, const float* a, const float* b, const uint32_t* n, const float* albedo,
                         const float* normal, const float* depth, uint32_t width, uint32_t rows, uint32_t level,
                         float threshold, float sigma_normal, float sigma_depth, uint32_t* list, uint32_t cap,
                         uint32_t* total, float* err, void* stream);
uint32_t gpu_adaptive_count(AdaptiveScratch* s, void* stream);  // waits for `stream`: the last select's total
// On the scratch's own buffers: n = value everywhere; the list's first `count` entries merged with m new samples per
// half from a_new, b_new; out = (A + B) / 2 (3 f32 per pixel) and samples = 2 n (device pointers).
void gpu_adaptive_fill(AdaptiveScratch* s, size_t pixels, uint32_t value, void* stream);
void gpu_adaptive_merge(AdaptiveScratch* s, uint32_t count, uint32_t m, void* stream);
void gpu_adaptive_finish(AdaptiveScratch* s, size_t pixels, float* out, uint32_t* samples, void* stream);
// First `count` draws of `lanes` consecutive streams starting at stream0 (tests).
struct JitCounts {
    uint64_t compiled, launches, failed, compile_ns, disk_hits, load_retries;
};
JitCounts gpu_jit_counts();  // scene-specialised kernels (jit.hip)
uint64_t gpu_jit_compile_only(const char* targs, std::string* log);
void gpu_rng_probe(uint32_t rng, uint64_t stream0, uint32_t lanes, uint32_t count, uint32_t sample, uint64_t* host_out);

}  // namespace nrt
