/*
 * nrt.h — C ABI of the MI355X-native renderer for nr-ray-tracer's per-pixel
 * path-tracing loop.
 *
 * The reference has no FFI: the path sits behind Rust generics/traits
 * (SURVEY.md §8b).  Each entry point below names the reference interface it
 * replaces; a Rust host binds them with one `extern "C"` block
 * (INTEGRATION.md).  Conventions:
 *   - every int-returning call returns NRT_OK (0) or a negative NRT_E_* code and
 *     never aborts the process; nrt_last_error() gives the message (thread-local);
 *   - the caller owns every buffer it passes; the library copies all inputs;
 *   - all structs are plain data; no torch / HIP types appear in signatures
 *     (streams are passed as void*).
 */
#ifndef NRT_H
#define NRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRT_ABI_VERSION 7

enum {
    NRT_OK = 0,
    NRT_E_INVALID = -1,     /* bad argument */
    NRT_E_LOAD = -2,        /* scene file / config error (anyhow::Error in the reference) */
    NRT_E_DEVICE = -3,      /* HIP error / no device */
    NRT_E_UNSUPPORTED = -4  /* feature outside the accelerated path (reserved; every reference scene feature renders) */
};

enum nrt_precision { NRT_PRECISION_F64 = 0, NRT_PRECISION_F32 = 1 };
enum nrt_rng { NRT_RNG_CHACHA8 = 0, NRT_RNG_PHILOX = 1 };
/* Traversal of the f32 kernel (the f64 kernel always walks the reference's BVH):
 *   BVH        the reference's BVH with instances kept (composed transforms), per lane;
 *   WORLD_LIST instances flattened to world space, every lane tests every primitive
 *              (six quads closing a box count as one slab test);
 *   WORLD_BVH  instances flattened, binned-SAH BVH, nearest-child-first with a per-lane stack.
 * AUTO picks WORLD_LIST when the scene flattens and makes at most NRT_WORLD_LIST_MAX
 * test units (nrt_scene_stats.world_prims), else WORLD_BVH when it flattens, else BVH.
 * The WORLD_* modes fail with NRT_E_INVALID on scenes that cannot flatten. */
enum nrt_trace { NRT_TRACE_AUTO = 0, NRT_TRACE_BVH = 1, NRT_TRACE_WORLD_LIST = 2, NRT_TRACE_WORLD_BVH = 3 };
#define NRT_WORLD_LIST_MAX 48

typedef struct nrt_scene nrt_scene;
typedef struct nrt_builder nrt_builder;

/* CameraConfig (packages/ray-tracer/src/cli.rs:157-270): each field optional,
 * present when its NRT_CC_* bit is set in `set`.  Angles in degrees. */
enum {
    NRT_CC_WIDTH = 1u << 0,
    NRT_CC_HEIGHT = 1u << 1,
    NRT_CC_ASPECT_RATIO = 1u << 2,
    NRT_CC_BACKGROUND_COLOR = 1u << 3,
    NRT_CC_LOOK_AT = 1u << 4,
    NRT_CC_LOOK_FROM = 1u << 5,
    NRT_CC_VIEW_UP = 1u << 6,
    NRT_CC_FOCAL_LENGTH = 1u << 7,
    NRT_CC_FIELD_OF_VIEW = 1u << 8,
    NRT_CC_DEFOCUS_ANGLE = 1u << 9,
    NRT_CC_FOCUS_DISTANCE = 1u << 10,
    NRT_CC_SAMPLES_PER_PIXEL = 1u << 11,
    NRT_CC_RAY_MAX_BOUNCES = 1u << 12
};

typedef struct {
    uint32_t set;
    uint32_t reserved;
    uint64_t width, height;
    double aspect_ratio;
    double background_color[3];
    double look_at[3];
    double look_from[3];
    double view_up[3];
    double focal_length; /* parsed, ignored — as in the reference (cli.rs:229) */
    double field_of_view;
    double defocus_angle;
    double focus_distance;
    uint64_t samples_per_pixel;
    uint64_t ray_max_bounces;
} nrt_camera_config;

/* CameraBuilder (lib/camera.rs:30-41); angles in radians. */
typedef struct {
    uint64_t width, height;
    double background_color[3];
    double look_from[3];
    double look_at[3];
    double view_up[3];
    double defocus_angle;
    double focus_dist;
    double field_of_view;
    uint64_t ray_max_bounces;
    uint64_t samples_per_pixel;
} nrt_camera_builder;

/* Camera after CameraBuilder::build (lib/camera.rs:205-227). */
typedef struct {
    uint64_t width, height;
    uint64_t samples_per_pixel;
    uint64_t ray_max_bounces;
    double background_color[3];
    double look_from[3];
    double defocus_disk_u[3];
    double defocus_disk_v[3];
    double pixel_delta_u[3];
    double pixel_delta_v[3];
    double top_left[3];
} nrt_camera;

typedef struct {
    uint32_t precision;  /* nrt_precision */
    uint32_t rng;        /* nrt_rng */
    int32_t device;      /* HIP device ordinal; -1 = current device (gpus >= 1: -1 = device 0) */
    uint32_t row_offset; /* render image rows y = row_offset + k*row_stride ... */
    uint32_t row_stride; /* ... (0 or 1: every row); output rows are compact */
    uint32_t trace;      /* nrt_trace (f32 kernel only) */
    /* 0: one device (`device`), the rows above.  N >= 1: the whole frame over the N devices
     * device .. device+N-1 of this process (Camera::render's one call over the whole machine,
     * lib/camera.rs:315-316): device first+r renders rows y = r (mod N) into its HBM,
     * one RCCL ncclGather (librccl, dlopen'ed; N = 1: a device copy, nothing to exchange) brings the
     * shards to the first device, which un-permutes them into the frame.  Needs row_offset 0 and row_stride <= 1; the frame is the
     * same bits as gpus = 0 (pixels and their RNG streams do not depend on the device).  The
     * scene owns the communicators and shard buffers (created on first use, freed with it). */
    uint32_t gpus;
    /* Philox only: the launch renders samples sample_offset .. sample_offset + spp - 1 of every pixel (spp =
     * the camera's samples_per_pixel) and divides their sum by spp.  A pixel's sample s draws the blocks
     * (pixel, s, step) whatever launch renders it, so windows over disjoint ranges are independent, and the
     * frames R(s0, m) of the windows [s0, s0 + m) compose: (a + n) R(0, a + n) = a R(0, a) + n R(a, n) up to
     * each frame's own rounding.  0: the frame of every earlier version, bit for bit.  The pixel jitter is on
     * when this launch's spp > 1, whatever the offset: a window of one sample goes through the pixel's
     * centre.  NRT_E_INVALID (before any device is touched): f32 with sample_offset + spp > 2^24 (the
     * Philox2x32 counter packs sample | step << 24), f64 with sample_offset + spp >= 2^32, and ChaCha8 with
     * a non-zero offset (the reference stream is sequential: where a window starts depends on the lengths
     * of the paths before it).  Row selection and gpus = N take it unchanged; nrt_render_aov* ignores it. */
    uint32_t sample_offset;
    /* Next-event estimation, f32 + Philox in the world-list and world-BVH modes (reference counterpart: none; the
     * expected frame is the reference's).  Non-zero: at every Lambertian hit of the ray with bounce index b, when
     * b + 1 < ray_max_bounces, one light is picked (probability P: area x the largest component of Le = intensity
     * x colour), one point y on it (quads and triangles uniform in area, a sphere uniform in the cone it subtends),
     * and one shadow ray x -> y adds  throughput x albedo x p_ref(n.w) x Le x W  when its closest hit is the light
     * itself.  p_ref is the density of the reference's scatter direction n + p / |p|^2 (not a cosine lobe: an eighth
     * of it lies below the surface), W = |n_l.w| area / (r^2 P) for a quad or triangle (two-sided) and
     * 2 pi (1 - cos theta_max) / P for a sphere.  The ray scattered from that hit then adds nothing when it ends
     * on a light by chance; camera rays and rays leaving a Metal or Dielectric count lights as before.  The
     * scatter draws keep their blocks; the light draws take Philox2x32 blocks of their own, step 127 + (b + 1).
     * Limit: a hit on or inside an emissive sphere gets no light from that sphere.
     * 0: every frame as without the field, bit for bit; a scene without lights renders the plain frame too.
     * Before any device is touched: NRT_E_INVALID for ChaCha8 (the reference stream has no such draws) and for
     * ray_max_bounces > 126; NRT_E_UNSUPPORTED for f64, the instance-BVH mode, gpus >= 1, and a scene with a
     * light that cannot be sampled (an emissive material whose texture is not a solid colour, a moving emissive
     * sphere, an emissive sphere the f32 kernels test in f64, more than 4096 lights: nrt_scene_stats.lights).
     * Row selection, sample_offset, nrt_render_pixels and nrt_render_adaptive take it unchanged; nrt_render_aov*
     * ignores it. */
    uint32_t direct_light;
} nrt_render_opts;

typedef struct {
    uint64_t nodes, prims, instances, xforms, materials, textures, texels; /* texels: of all image textures */
    uint32_t trees, max_instance_depth;
    uint64_t device_bytes; /* HBM bytes of the flattened scene on one device */
    uint64_t world_prims;  /* world-list test units after flattening instances to world space: primitives,
                              with six quads closing a box counted once (0: not flattenable) */
    uint32_t coplanar_pairs; /* overlapping coplanar surface pairs (their hits tie in the reference) */
    uint32_t world_list_ok;  /* 1: the world list resolves every such tie as the reference does
                                (else AUTO takes the world BVH, which compares tie keys) */
    uint32_t exact_mode;     /* traversal of the f64 reference-exact kernel (NRT_EXACT_*) */
    uint32_t texel_formats;  /* image textures' storage formats, bit 1 << f for each format f used:
                                0 RGB32F (12 B per texel), 1 RGBA8 (4), 2 RGB8T (3), 3 PAL16 (2 + palettes) */
    /* HBM bytes of the texel array: image textures as stored (PAL16, the default for file images
     * whose bands fit: a 2-byte palette index per texel in 8 x 8 tiles plus an RGBA8 palette per
     * band; else RGB8T, 3 B per texel in 128-B tiles of 8 x 5; RGBA8 tiles; RGB32F for constructor
     * images with values other than k/255) plus the Perlin permutation tables of Noise / Marble */
    uint64_t texel_bytes;
    uint32_t lights; /* primitives whose material is a DiffuseLight (instances flattened: one per placement) */
} nrt_scene_stats;
/* Exact-kernel traversal (same closest hit and tie-break as BVH::hit, object.rs:89-121):
 *   BVH      the reference tree, box by box
 *   ALL      every primitive in the tree's depth-first order, no boxes (at most 48 primitives)
 *   WORLD    the f32 world BVH culls (conservatively), the reference tests decide */
enum nrt_exact_mode { NRT_EXACT_BVH = 0, NRT_EXACT_ALL = 1, NRT_EXACT_WORLD = 2 };

typedef void (*nrt_progress_fn)(void* user, uint64_t pixels_done);

/* ---- library ---------------------------------------------------------- */
int nrt_abi_version(void);
/* sha256 prefix of the library's sources it was built from (build provenance; no reference
 * counterpart) */
const char* nrt_build_id(void);
/* Scene-specialised kernels (built with hiprtc, loaded lazily, when a scene is first rendered
 * in an f32 world mode; NRT_JIT=0 turns them off, NRT_JIT=require makes a failed build an
 * error of the render call instead of a fallback to the generic kernel).  The first such render
 * of a scene pays the compile (0.2-0.5 s) inside the render call, unless the on-disk code-object
 * cache holds it (NRT_JIT_CACHE = a directory, default $XDG_CACHE_HOME/nrt-jit or
 * ~/.cache/nrt-jit; "0" turns it off): keyed by the library's build id, a hash of the embedded
 * device headers, the hiprtc and HIP runtime versions, the architecture, the template arguments
 * (the scene's geometry signature and its shading signature: the material kinds its materials
 * use and the camera's mode, defocus on or off, spp > 1 and a sample window past 0, so a render with another
 * camera mode builds or loads another kernel) and the compile options, written atomically and verified on load.
 * out[0] = kernels built by hiprtc in this process, out[1] = renders that used a specialised
 * kernel, out[2] = builds that failed (the generic kernel rendered instead: slower, the same
 * frame bit for bit), out[3] = compile + load wall time in ns, out[4] = code objects taken from
 * the disk cache, out[5] = module loads that failed and were retried; the first min(n, 6) are
 * written.  No reference counterpart. */
int nrt_jit_stats(uint64_t* out, size_t n);
/* Tests: compile render_kernel<targs> with hiprtc from the embedded headers, no GPU needed
 * (nothing is loaded); *code_bytes = the code object's size. */
int nrt_debug_jit_compile(const char* targs, uint64_t* code_bytes);
const char* nrt_last_error(void);   /* thread-local; message text mirrors anyhow's */
int nrt_device_count(void);

/* ---- camera (lib/camera.rs:162-203, 94-159; app cli.rs:316-402) --------- */
void nrt_camera_builder_default(nrt_camera_builder* out);           /* CameraBuilder::default */
int nrt_camera_build(const nrt_camera_builder* b, nrt_camera* out);  /* CameraBuilder::build */
/* CameraConfig::try_update onto a builder (image-size rules, degrees->radians) */
int nrt_camera_config_apply(const nrt_camera_config* cfg, nrt_camera_builder* b);

/* ---- scene from file: SceneConfig::try_load_scene + merge_with + try_build
 *      (app scene_config.rs:475-496, render.rs:107-111).  Relative paths inside
 *      the file (nested scenes, textures) resolve against the process CWD, as in
 *      the reference.  `overrides` may be NULL. */
int nrt_scene_load(const char* path, const nrt_camera_config* overrides, nrt_scene** out, nrt_camera* camera);
/* The same with load flags: NRT_LOAD_LEGACY_SCHEMA also accepts the legacy index schema of
 * scenes/triangles.toml (integer texture / material references, `objects`), mapped onto the
 * current one with ids "0", "1", ... (what `create triangles` writes today, create/triangles.rs).
 * Without it the file fails to load (NRT_E_LOAD), as in the reference. */
enum { NRT_LOAD_LEGACY_SCHEMA = 1u << 0 };
int nrt_scene_load_ex(const char* path, const nrt_camera_config* overrides, uint32_t flags, nrt_scene** out,
                      nrt_camera* camera);

/* ---- scene from the library constructors (the Hitable/Material/Texture
 *      trait surface of nr-ray-tracer-lib).  Handles are small non-negative
 *      integers (negative = error). */
nrt_builder* nrt_builder_new(void);
void nrt_builder_free(nrt_builder* b);
int32_t nrt_texture_solid(nrt_builder* b, const double color[3]);                      /* SolidColor::new */
int32_t nrt_texture_image(nrt_builder* b, uint32_t w, uint32_t h, const float* rgb);   /* Image (Rgb32F texels) */
int32_t nrt_texture_image_file(nrt_builder* b, const char* path);                      /* Image::try_from_path */
int32_t nrt_texture_checker(nrt_builder* b, int32_t even, int32_t odd, double scale);  /* CheckerBuilder */
/* PerlinRidgedNoiseBuilder (lib/textures/noise.rs:30-101) and MarbleBuilder (lib/textures/marble.rs:24-60):
 * each builder field is an Option, present when its NRT_NOISE_* bit is set in `set`; absent fields take the
 * builder's defaults (seed 0; octaves 1, clamped to [1, 32] by Fbm::set_octaves; frequency 1; lacunarity
 * 2*pi/3; persistence 0.5; Marble: 7 octaves and the default lacunarity / persistence, only seed and
 * frequency read).  get_color: |Fbm<Perlin>|(p) (Noise), (1 + sin(frequency * p.z + 10 |Fbm|(p))) / 2
 * (Marble), grey, at the world-space hit point. */
enum {
    NRT_NOISE_SEED = 1u << 0,
    NRT_NOISE_OCTAVES = 1u << 1,
    NRT_NOISE_FREQUENCY = 1u << 2,
    NRT_NOISE_LACUNARITY = 1u << 3,
    NRT_NOISE_PERSISTENCE = 1u << 4
};
int32_t nrt_texture_noise(nrt_builder* b, uint32_t set, uint32_t seed, uint64_t octaves, double frequency,
                          double lacunarity, double persistence);
int32_t nrt_texture_marble(nrt_builder* b, uint32_t set, uint32_t seed, double frequency);
int32_t nrt_material_lambertian(nrt_builder* b, int32_t texture);                       /* Lambertian::with_texture */
int32_t nrt_material_metal(nrt_builder* b, double fuzz, int32_t texture);               /* MetalBuilder */
int32_t nrt_material_dielectric(nrt_builder* b, double refraction_index);               /* Dielectric::new */
int32_t nrt_material_diffuse_light(nrt_builder* b, double intensity, int32_t texture);  /* DiffuseLightBuilder */
int32_t nrt_object_sphere(nrt_builder* b, const double center[3], double radius, int32_t material); /* SphereBuilder */
/* SphereBuilder::with_speed (lib/objects/sphere.rs:45-50): centre(time) = center + time * speed for the
 * ray's time in [0, 1) (sphere.rs:110-111, camera.rs:264); the box spans both end positions (sphere.rs:72-84) */
int32_t nrt_object_sphere_moving(nrt_builder* b, const double center[3], const double speed[3], double radius,
                                 int32_t material);
int32_t nrt_object_quad(nrt_builder* b, const double p[3], const double u[3], const double v[3], int32_t material);
int32_t nrt_object_triangle(nrt_builder* b, const double p[3], const double u[3], const double v[3], int32_t material);
int32_t nrt_object_bvh(nrt_builder* b, const int32_t* objects, size_t count);          /* BVH::from */
int32_t nrt_object_translate(nrt_builder* b, int32_t object, const double offset[3]);  /* Translate::new */
int32_t nrt_object_rotate_x(nrt_builder* b, int32_t object, double angle);             /* Rotate::axis_x */
int32_t nrt_object_rotate_y(nrt_builder* b, int32_t object, double angle);             /* Rotate::axis_y */
int32_t nrt_object_rotate_z(nrt_builder* b, int32_t object, double angle);             /* Rotate::axis_z */
int32_t nrt_object_scale(nrt_builder* b, int32_t object, const double scale[3]);       /* Scale::new */
/* Scene { objects: BVH } (lib/scene.rs:6-10); `bvh` must come from nrt_object_bvh. */
int nrt_builder_finish(nrt_builder* b, int32_t bvh, nrt_scene** out);

/* ---- render: Scene::render / Camera::render (lib/scene.rs:13-18, lib/camera.rs:302-343)
 * out_rgb: caller-owned, rows*width*3 f32, row-major (Rgb32FImage layout), where
 * rows = the rows selected by opts (all rows by default).  Synchronous.
 * progress (may be NULL) is called from the calling thread with the number of
 * pixels finished so far, at launch granularity. */
int nrt_render(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts, float* out_rgb,
               size_t out_len, nrt_progress_fn progress, void* user);
/* Same, into device memory on `hip_stream` (hipStream_t, NULL = default stream);
 * asynchronous: returns after enqueueing. */
int nrt_render_device(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                      float* dev_out_rgb, size_t out_len, void* hip_stream);
/* With opts->gpus = N >= 1: dev_out_rgb (W*H*3 f32) and hip_stream belong to the first device
 * (a stream of another device: NRT_E_INVALID); every device's render and the gather are enqueued
 * and the call returns.  The first device's gather and the un-permute run on hip_stream itself,
 * after its prior work, so the library adds only its render streams to the caller's.  Consecutive
 * calls pipeline: frame k+1's renders may start while frame k's last paths, gather and un-permute
 * run. */
/* Everything a render of (scene, camera, opts) needs before its first launch, done now (ABI 7): the
 * upload to the device, and with opts->gpus = N the upload to every device, the RCCL communicators
 * and the shard / staging buffers, so a timed first render (render.rs:57-62) pays none of it.
 * NRT_E_UNSUPPORTED when gpus >= 2 and librccl (ncclGather, ncclCommInitAll) is not usable: a host
 * may then render row shards per device itself (nrt_render_opts row_offset / row_stride). */
int nrt_render_prepare(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts);
/* HIP-event times (ms) of the scene's last gpus >= 1 render (waits for it): out[d] = the render
 * launch on device first+d, d < N (begin to end; consecutive frames overlap, so this can include the
 * previous frame's tail); out[N] = the gather + un-permute on the first device (from its own render's
 * end, so the slowest device's lag is in it); out[N+1] = the device time per frame since the previous
 * call that wrote it: from the first device's render start of that window's first frame to the last
 * frame's completion (gather + un-permute done), over the frames (0 with fewer than two); a call that
 * writes out[N+1] starts a new window.  *count = N + 2; at most n written. */
int nrt_render_timings(const nrt_scene* scene, float* out, size_t n, size_t* count);
/* ---- feature buffers and the edge-avoiding filter (reference counterpart: none; the reference
 *      writes the Monte-Carlo frame as it is) */
typedef struct {
    uint32_t iterations; /* a-trous passes K, 1..5; 0 = 5.  Pass i has step 2^i */
    float sigma_color, sigma_normal, sigma_depth; /* <= 0: the defaults 0.6, 0.3, 0.5 */
} nrt_denoise_opts;
/* First-hit feature buffers of the rows opts selects (reference counterpart: none): one primary
 * ray per pixel, origin look_from, direction top_left + x pixel_delta_u + y pixel_delta_v -
 * look_from (no jitter, no defocus, time 0), traced in f32 in the mode opts->trace names (AUTO as
 * the render; precision and rng are not read).  albedo, normal: 3 f32 per pixel, depth: 1, row-major,
 * each with room for n_pixels >= rows * width pixels; any of the three may be NULL.
 *   albedo  Lambertian / Metal / DiffuseLight: the texture's colour at the hit (a light's is not
 *           scaled by its intensity); Dielectric: (1, 1, 1); miss: the camera's background colour
 *   normal  the hit record's unit normal, facing the ray; miss: (0, 0, 0)
 *   depth   distance from look_from to the hit point; miss: 0 (no hit has it: t >= 0.001)
 * Host buffers, synchronous.  opts->gpus >= 1: NRT_E_INVALID (one device renders the pass). */
int nrt_render_aov(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts, float* albedo,
                   float* normal, float* depth, size_t n_pixels);
/* Same, into device memory on `hip_stream` (NULL = default stream); asynchronous (reference
 * counterpart: none). */
int nrt_render_aov_device(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                          float* dev_albedo, float* dev_normal, float* dev_depth, size_t n_pixels, void* hip_stream);
/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of a `rows` x `width` frame (reference
 * counterpart: none).  With a = max(albedo, 1e-3), D_0 = colour / a, and for pass i = 0 .. K-1 the
 * step s = 2^i, taps q = p + s (dx, dy) with dx, dy in -2 .. 2 (those outside the image skipped) and
 * h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   e(p, q) = |D_i(p) - D_i(q)|^2 / (sigma_color 2^-i)^2 + |N(p) - N(q)|^2 / sigma_normal^2
 *             + (Z(p) - Z(q))^2 / sigma_depth^2
 *   D_{i+1}(p) = sum_q h[dx] h[dy] exp(-e) D_i(q) / sum_q h[dx] h[dy] exp(-e)
 * out = D_K a.  colour, albedo, normal, out: 3 f32 per pixel, depth: 1; out may be colour (in
 * place), no other overlap.  dopts NULL = the defaults.  The result is a pure function of the
 * inputs, the same bits from run to run.  Needs no scene: host buffers, device scratch for the
 * call's duration on `device` (-1 = the current device), synchronous. */
int nrt_denoise(const float* colour, const float* albedo, const float* normal, const float* depth, uint32_t width,
                uint32_t rows, const nrt_denoise_opts* dopts, int32_t device, float* out);
/* Same over device memory on the device that holds it (`device`, -1 = current), K launches enqueued on
 * `hip_stream`, asynchronous (reference counterpart: none).  The scene owns the scratch (two colour
 * buffers and the packed guide records, 40 B per pixel; created on first use, kept for the next
 * frame, freed with the scene): calls on one scene and device must be ordered by their streams. */
int nrt_denoise_device(const nrt_scene* scene, const float* dev_colour, const float* dev_albedo,
                       const float* dev_normal, const float* dev_depth, uint32_t width, uint32_t rows,
                       const nrt_denoise_opts* dopts, int32_t device, float* dev_out, void* hip_stream);
typedef struct {
    uint32_t iterations; /* a-trous passes K, 1..5; 0 = 5.  Pass i has step 2^i */
    float sigma_luminance, sigma_normal, sigma_depth; /* <= 0: the defaults 4, 0.3, 0.5 */
} nrt_denoise_vg_opts;
/* Variance-guided a-trous filter: the spatial filter of SVGF (Schied et al. 2017) with its spatial
 * variance estimate (reference counterpart: none).  a, D_0, the steps, the taps and h as for
 * nrt_denoise; lum(x) = 0.2126 x_r + 0.7152 x_g + 0.0722 x_b, l_i = lum(D_i),
 *   g(p, q) = |N(p) - N(q)|^2 / sigma_normal^2 + (Z(p) - Z(q))^2 / sigma_depth^2,
 * taps outside the image skipped in every sum.  Over q = p + (dx, dy), |dx|, |dy| <= 3, with
 * w = exp(-g(p, q)) and d = l_0(q) - l_0(p):
 *   Var_0(p) = max(0, sum w d^2 / sum w - (sum w d / sum w)^2)
 * Pass i = 0 .. K-1, with g3 = (1/4, 1/2, 1/4) over the 3 x 3 pixels at distance 1 (not s):
 *   sigma(p) = sqrt(sum g3[dx] g3[dy] Var_i(q) / sum g3[dx] g3[dy])
 *   e(p, q) = |l_i(p) - l_i(q)| / (sigma_luminance sigma(p) + 1e-6) + g(p, q)
 *   w = h[dx] h[dy] exp(-e),  D_{i+1}(p) = sum w D_i(q) / sum w,  Var_{i+1}(p) = sum w^2 Var_i(q) / (sum w)^2
 * out = D_K a; out_variance (1 f32 per pixel, may be NULL) = Var_K, the variance of the demodulated
 * luminance.  Buffers, overlap (out may be colour, for every K), dopts NULL, determinism, device and
 * synchrony as nrt_denoise. */
int nrt_denoise_vg(const float* colour, const float* albedo, const float* normal, const float* depth, uint32_t width,
                   uint32_t rows, const nrt_denoise_vg_opts* dopts, int32_t device, float* out, float* out_variance);
/* Same over device memory, K + 1 launches enqueued on `hip_stream`, asynchronous (reference
 * counterpart: none).  The scene owns the scratch (two colour-and-variance buffers and the packed
 * guide records, 48 B per pixel, apart from nrt_denoise_device's), under nrt_denoise_device's rules. */
int nrt_denoise_vg_device(const nrt_scene* scene, const float* dev_colour, const float* dev_albedo,
                          const float* dev_normal, const float* dev_depth, uint32_t width, uint32_t rows,
                          const nrt_denoise_vg_opts* dopts, int32_t device, float* dev_out, float* dev_out_variance,
                          void* hip_stream);
/* The variance-guided filter with a dual-buffer variance estimate (reference counterpart: none).  colour_a and
 * colour_b are two frames A, B of one camera over disjoint sample windows of equal length (nrt_render_opts.
 * sample_offset), so their noise is independent and their mean is the frame over both windows.  a, lum, g(p, q), the
 * passes and the sigmas as for nrt_denoise_vg:
 *   D_0(p)   = ((A + B) / 2) / a                        per channel
 *   delta(p) = lum((A - B) / a) / 2                     per-channel IEEE divisions, then lum
 *   Var_0(p) = sum_q w(p, q) delta(q)^2 / sum_q w(p, q),  q = p + (dx, dy), |dx|, |dy| <= 3, w = exp(-g(p, q)),
 *              taps outside the image skipped
 * then nrt_denoise_vg's K passes from (D_0, Var_0): out = D_K a, out_variance (may be NULL) = Var_K.  For independent
 * halves E[delta^2] is the variance of lum(D_0): delta^2 is a one-degree-of-freedom estimate of the noise alone, which
 * the guide-weighted window pools; shading features the guides do not see (shadow edges, reflections) are in A and B
 * alike and cancel, where nrt_denoise_vg's spatial spread counts them as noise.  No luminance term enters w: an edge
 * in the image is not evidence of noise.  A == B gives a variance of exactly 0 everywhere.  Buffers as
 * nrt_denoise_vg's; out may be colour_a or colour_b (in place), no other overlap (NRT_E_INVALID).  dopts NULL,
 * determinism, device and synchrony as nrt_denoise. */
int nrt_denoise_vg_dual(const float* colour_a, const float* colour_b, const float* albedo, const float* normal,
                        const float* depth, uint32_t width, uint32_t rows, const nrt_denoise_vg_opts* dopts,
                        int32_t device, float* out, float* out_variance);
/* Same over device memory, K + 1 launches enqueued on `hip_stream`, asynchronous (reference counterpart: none), on the
 * scene's variance-guided scratch (nrt_denoise_vg_device's, under its rules). */
int nrt_denoise_vg_dual_device(const nrt_scene* scene, const float* dev_colour_a, const float* dev_colour_b,
                               const float* dev_albedo, const float* dev_normal, const float* dev_depth, uint32_t width,
                               uint32_t rows, const nrt_denoise_vg_opts* dopts, int32_t device, float* dev_out,
                               float* dev_out_variance, void* hip_stream);
/* ---- adaptive sampling: a render over a list of pixels, an error estimate that selects pixels, and the loop that
 *      refines a frame until its error is below a threshold (reference counterpart: none; the reference gives every
 *      pixel the same samples).  Philox only, one device, whole frames. */
/* The pixels pixels[0 .. n), linear indices y * width + x, rendered as nrt_render renders them: out_rgb[3 k ..] is,
 * bit for bit, the pixel pixels[k] of the frame nrt_render gives for the same camera and opts (the same RNG blocks,
 * jitter rule, pixel sums and sample window opts->sample_offset), so n * 3 floats in list order.  An index may
 * repeat.  NRT_E_INVALID before any device is touched: opts NULL or rng = ChaCha8, a row subset (row_offset,
 * row_stride > 1), gpus >= 1, an index >= width * height.  n = 0: NRT_OK, nothing launched.  Host buffers,
 * synchronous. */
int nrt_render_pixels(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                      const uint32_t* pixels, size_t n, float* out_rgb);
/* Same over device memory on `hip_stream` (NULL = default stream), asynchronous; the indices are the caller's to
 * keep below width * height (they are not read on the host). */
int nrt_render_pixels_device(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                             const uint32_t* dev_pixels, size_t n, float* dev_out_rgb, void* hip_stream);
typedef struct {
    float threshold;      /* a pixel takes more samples until its relative error is below this; >= 0 */
    uint32_t min_samples; /* samples every pixel gets (nrt_render_adaptive); 0 = max(4, samples_per_pixel / 8) */
    float sigma_normal, sigma_depth; /* <= 0: the defaults 0.3, 0.5 */
} nrt_adaptive_opts;
/* Which pixels need more samples.  Per pixel: the means A, B of two halves of its samples over disjoint windows
 * (3 f32 each) and n = half_samples (u32), the samples each half holds.  With a = max(albedo, 1e-3) and lum, g(p, q),
 * the 7 x 7 window and the skipped outside taps as for nrt_denoise_vg_dual:
 *   delta(q) = lum((A - B) / a) / 2            v(q) = n(q) delta(q)^2
 *   Var(p)   = (sum_q w v(q) / sum_q w) / n(p),   w = exp(-g(p, q))
 *   err(p)   = sqrt(Var(p)) / (lum(((A + B) / 2) / a) + 0.01)
 *   select p  iff  n(p) == level  and  err(p) >= threshold
 * v is a per-sample variance, so neighbours that hold other sample counts pool without bias; / n(p) makes it the
 * variance of p's mean.  The comparison is not strict: threshold 0 selects every pixel of the level, also one whose
 * halves agree exactly (err = 0: a pixel that sees only the background), so 0 renders the whole frame to the cap.
 * pixels_out receives the selected pixels' linear indices, 32 x 8 tiles in row-major tile
 * order and pixels row-major inside a tile (a pure function of the inputs; at most `cap` entries are written),
 * *count their number, which may exceed cap; error_out (1 f32 per pixel, may be NULL) err(p) of every pixel.
 * aopts->min_samples is not read.  Host buffers, device scratch for the call's duration on `device` (-1 = the
 * current device), synchronous. */
int nrt_adaptive_select(const float* a, const float* b, const uint32_t* half_samples, const float* albedo,
                        const float* normal, const float* depth, uint32_t width, uint32_t rows, uint32_t level,
                        const nrt_adaptive_opts* aopts, int32_t device, uint32_t* pixels_out, size_t cap, uint32_t* count,
                        float* error_out);
/* Same over device memory (dev_count: one u32 on the device), three launches enqueued on `hip_stream`, asynchronous.
 * The scene owns the scratch (nrt_render_adaptive's: created on first use, kept, freed with the scene), under
 * nrt_denoise_device's rules. */
int nrt_adaptive_select_device(const nrt_scene* scene, const float* dev_a, const float* dev_b,
                               const uint32_t* dev_half_samples, const float* dev_albedo, const float* dev_normal,
                               const float* dev_depth, uint32_t width, uint32_t rows, uint32_t level,
                               const nrt_adaptive_opts* aopts, int32_t device, uint32_t* dev_pixels_out, size_t cap,
                               uint32_t* dev_count, float* dev_error_out, void* hip_stream);
/* Render until err(p) < aopts->threshold, at most S = camera->samples_per_pixel samples per pixel.  H = S / 2,
 * s0 = opts->sample_offset, R(s, m) = the frame of the window [s, s + m):
 *   features: nrt_render_aov's buffers, once
 *   level 0:  A = R(s0, n0), B = R(s0 + H, n0), n = n0 = min_samples / 2 everywhere
 *   while n_cur < H: select at level n_cur (stop when nothing is selected); m = n_cur; the selected pixels' windows
 *             [s0 + n_cur, + m) and [s0 + H + n_cur, + m) by two list renders A', B'; per channel
 *             A = (n A + m A') / (n + m) in f64 rounded once to f32, the same for B; n += m; n_cur += m
 *   out = (A + B) * 0.5f; out_samples (u32 per pixel, may be NULL) = 2 n; out_a, out_b (3 f32 per pixel, may be
 *   NULL) = A, B, two frames nrt_denoise_vg_dual accepts
 * A pixel not selected at its level is never selected again, so every launch has one window; a pixel that reaches
 * S has drawn exactly the samples [s0, s0 + S) of nrt_render.  NRT_E_INVALID before any device is touched: opts NULL
 * or ChaCha8, a row subset, gpus >= 1, aopts NULL or a threshold not >= 0, S odd, min_samples odd or < 4 (every
 * window must jitter), S / min_samples not a power of two, sample_offset + S past nrt_render_opts.sample_offset's
 * limits.  out_len >= width * height * 3.  The scene owns the scratch (84 B per pixel).  Synchronous. */
int nrt_render_adaptive(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                        const nrt_adaptive_opts* aopts, float* out_rgb, size_t out_len, uint32_t* out_samples,
                        float* out_a, float* out_b);
/* ---- temporal accumulation in front of the variance-guided filter: SVGF (Schied et al. 2017) whole
 *      (reference counterpart: none).  The scene is static between frames, so reprojection is a
 *      function of the two cameras and the depth buffer alone. */
typedef struct nrt_history nrt_history;
typedef struct {
    uint32_t iterations; /* a-trous passes K, 2..5; 0 = 5 (the history takes the first pass's output) */
    float sigma_luminance, sigma_normal, sigma_depth; /* <= 0: the defaults 4, 0.3, 0.5 */
    float alpha_min; /* <= 0: 0.2 */
    float tau_z;     /* <= 0: 0.1 */
    float tau_n;     /* <= 0: 0.9 */
} nrt_denoise_temporal_opts;
/* A history of `width` x `rows` frames on `device` (-1 = the device current at the first frame).  It
 * owns every buffer, state and work: 112 B per pixel, allocated by the first frame (NULL: a zero size). */
nrt_history* nrt_history_new(uint32_t width, uint32_t rows, int32_t device);
void nrt_history_free(nrt_history* history);
/* The next frame's history is invalid at every pixel. */
int nrt_history_reset(nrt_history* history);
/* a, D = colour / a, lum, g(p, q), h, the steps, the passes and Var_0 as for nrt_denoise_vg.  The
 * history holds, of the previous frame ('): its camera, its guide records N', Z', its colour history H'
 * (rgb), its luminance moments m1', m2' and an integer history length n'.  Frame k with `camera`, at
 * pixel p = (x, y), l = lum(D(p)):
 *   d = top_left + x pixel_delta_u + y pixel_delta_v - look_from,  P = look_from + Z(p) d / |d|,
 *   r = P - look_from',  (A, B, Cc) = M'^-1 r with the columns of M' pixel_delta_u', pixel_delta_v',
 *   top_left' - look_from';  u = A / Cc, v = B / Cc, z' = |r|.
 * The host inverts M' in f64 (singular: NRT_E_INVALID) and hands the kernel f32 constants of the
 * equivalent form, with k = Z(p) / |d| and M's columns those of this camera,
 *   (A, B, Cc) = k (x, y, 1) + k M'^-1 (M - M') (x, y, 1) + M'^-1 (look_from - look_from'),
 * which makes u = x, v = y exact for equal cameras.  Taps q = (floor(u) + i, floor(v) + j), i, j in
 * {0, 1}, with the bilinear weights b_q of (u, v); a tap is valid when it lies in the image, Z'(q) > 0,
 * |Z'(q) - z'| <= tau_z z' and N'(q) . N(p) >= tau_n; sb = the sum of b_q over the valid taps.  The
 * history of p is valid when the history object holds a frame, Z(p) > 0, Cc > 0 and sb >= 0.01:
 *   Hh, M1, M2 = sum b_q (H', m1', m2')(q) / sb over the valid taps,
 *   n = min(1 + min over the valid taps of n'(q), 255),  alpha = max(alpha_min, 1 / n),
 *   I(p) = Hh + alpha (D(p) - Hh),  m1 = M1 + alpha (l - M1),  m2 = M2 + alpha (l^2 - M2);
 * otherwise I = D, m1 = l, m2 = l^2, n = 1.  The variance:
 *   V(p) = max(0, m2 - m1^2) when n >= 4, else Var_0(p) / n
 * (the frame's variance over the frames averaged is the variance of their mean; with alpha >= 1 / n the
 * blend is that mean for n < 4).  Then nrt_denoise_vg's K passes from (I, V) in place of (D_0, Var_0):
 * out = D_K a, out_variance = Var_K.  The new history: H = D_1.rgb (the first pass's output, SVGF's
 * feedback: K >= 2), m1, m2, n as above, N, Z and the camera of this frame.  The history length is an
 * integer minimum, not a bilinear mix, so the n >= 4 branch never sits on a rounding edge.
 * Host buffers as nrt_denoise_vg's (out may be colour; out_variance, 1 f32 per pixel, may be NULL and
 * overlaps nothing; no other overlap), synchronous.  NRT_E_INVALID: a camera whose size is not the
 * history's, K = 1 or K > 5, an overlap; NRT_E_DEVICE: no usable device.  No atomics, every sum by one
 * lane in one order: a pure function of the frames so far, the same bits from run to run. */
int nrt_denoise_temporal(nrt_history* history, const nrt_camera* camera, const float* colour, const float* albedo,
                         const float* normal, const float* depth, const nrt_denoise_temporal_opts* opts, float* out,
                         float* out_variance);
/* Same over device memory on the history's device, K + 1 launches enqueued on `hip_stream`,
 * asynchronous: calls on one history must be ordered by their streams. */
int nrt_denoise_temporal_device(nrt_history* history, const nrt_camera* camera, const float* dev_colour,
                                const float* dev_albedo, const float* dev_normal, const float* dev_depth,
                                const nrt_denoise_temporal_opts* opts, float* dev_out, float* dev_out_variance,
                                void* hip_stream);
/* The last frame's m1, m2 (moments: 2 f32 per pixel) and n (length: 1 f32 per pixel) to host memory,
 * after the device has finished; either pointer may be NULL.  NRT_E_INVALID before the first frame. */
int nrt_history_read(nrt_history* history, float* moments, float* length);

/* Number of rows selected by opts for an image of `height` rows. */
uint32_t nrt_rows_selected(uint32_t height, const nrt_render_opts* opts);
/* Upload the flattened scene to `device` now (otherwise done on first render). */
int nrt_scene_upload(nrt_scene* scene, int32_t device);

int nrt_scene_stats_get(const nrt_scene* scene, nrt_scene_stats* out);
/* Canonical text dump of the scene graph (BVH, boxes, transforms, materials) in
 * hex floats; *needed = bytes incl. NUL.  Used by parity tests. */
int nrt_scene_dump(const nrt_scene* scene, char* buf, size_t cap, size_t* needed);
void nrt_scene_destroy(nrt_scene* scene);

/* Image::try_from_path -> into_rgb32f (lib/textures/image.rs:24-28): decode an image file
 * (baseline JPEG) to W*H*3 f32 in [0, 1].  Call with rgb = NULL to get the size. */
int nrt_image_load(const char* path, uint32_t* width, uint32_t* height, float* rgb, size_t cap);

/* gamma_correction + to_rgb8 (lib/image.rs:53-57; image crate Rgb32F->Rgb8). */
int nrt_image_to_rgb8(const float* rgb, size_t n_floats, float gamma, uint8_t* out);

/* Tests: first `count` next_u64 draws of `lanes` consecutive pixel streams
 * (rng 0 ChaCha8: stream = pixel index, below 2^32 as every image pixel's: stream0 + lanes > 2^32 - 1
 * is NRT_E_INVALID; rng 1 Philox4x32-10: counter (pixel, sample, pair)),
 * or with rng 2 the f32 render loop's Philox2x32-10 blocks: word k of lane l = the block
 * of (pixel stream0 + l, sample, step k), lo | hi << 32 (count <= 256, sample < 2^24). */
int nrt_debug_rng(uint32_t rng, uint64_t stream0, uint32_t lanes, uint32_t count, uint32_t sample, uint64_t* out);

/* Tests: the 256-entry permutation table of the Perlin source for `seed` (noise 0.9.0
 * PermutationTable::new, used by the Noise / Marble textures, lib/textures/noise.rs:85-92). */
int nrt_debug_perlin_permutation(uint32_t seed, uint8_t* out);

/* Diagnostics: one render with per-wave s_memtime stamps; out[0..4] = {loop
 * iterations, camera-ray cycles, trace cycles, shading cycles, waves} summed over
 * waves, and with n >= 8 out[5..7] = the shading cycles split into {hit record +
 * material, sample claim + Philox block, scatter / camera ray + accumulate}.  With
 * rng = Philox, camera rays are part of shading and out[1] counts the lane-iterations
 * that shaded a path instead.  Slower than nrt_render; never timed. */
int nrt_debug_phase_profile(const nrt_scene* scene, const nrt_camera* camera, const nrt_render_opts* opts,
                            uint64_t* out, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* NRT_H */
