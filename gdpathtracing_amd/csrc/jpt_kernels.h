// jpt_kernels.h -- what the host layer (jpt_capi.cpp, jpt_scene_update.cpp, jpt_lighting.cpp, jpt_primary.cpp) sees of the device code, and the two values a
// render's launches read: its Lighting and its PrimaryRays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "jpt_nodeq.h"
#include "jpt_bake.h"
#include "jpt_camera.h"
#include "jpt_lens.h"
#include "jpt_probe.h"
#include "jpt_reflection.h"
#include "jpt_shade.h"
#include "jpt_skin.h"
#include "jpt_sky.h"
#include "jpt_types.h"

namespace jpt {

constexpr int kStripRows = 8;  // screen partition granule (jpt_set_partition)
constexpr int kMaxBounces = 64;  // the largest max_bounces (jpt_set_params)
constexpr int kMaxGroups = 4;    // the most frame groups a render is split into (launch_wf2_render)

// Runtime flags as template arguments: with_consts<N0, N1, ...>(f, v0, v1, ...) calls f with one constant per flag,
// std::bool_constant<v != 0> for N == 2 and std::integral_constant<int, v> otherwise.  Every v must lie in [0, N); only the
// values a launcher passes are instantiated.
template <int N, int V = 0, typename F>
inline void with_const(int v, F&& f)
{
    if constexpr (V + 1 < N) {
        if (v != V) return with_const<N, V + 1>(v, f);
    }
    if constexpr (N == 2) f(std::bool_constant<V != 0>{});
    else f(std::integral_constant<int, V>{});
}
template <int N, int... Ns, typename F, typename... Vs>
inline void with_consts(F&& f, int v, Vs... rest)
{
    with_const<N>(v, [&](auto k) {
        if constexpr (sizeof...(Ns) == 0) f(k);
        else with_consts<Ns...>([&](auto... ks) { f(k, ks...); }, rest...);
    });
}

struct DevCounters {  // SURVEY.md 8(d) event counters
    unsigned long long rays, blas_expand, tri_tests, tlas_expand, inst_visits, shaded_hits;
    // wave-level phase statistics of the tracing kernels (counting builds only): how many times a phase ran
    // in a wave and how many lanes took part -- [0] rounds, [1] node iterations, [2] lanes in them, [3] leaf
    // phases, [4] lanes in them, [5] instance phases, [6] lanes in them, [7] primary rays finished by the sky cull
    unsigned long long phase[8];
    // ... and the length of the walks: the most record steps (internal records + leaves + instance entries) any one ray took, and
    // how many rays took < 16, < 64, < 256, < 1024, < 4096, < 16384, < 65536, more (a launch cannot end before its longest ray)
    unsigned long long walk_max;
    unsigned long long walk_hist[8];
    // path vertices that go on with a throughput of exactly (0, 0, 0) (jpt_stats.zero_throughput)
    unsigned long long zero_thr;
};

struct FrameParams {
    int32_t width, height;      // full image (Params.width/height, main.glsl:103-104)
    int32_t local_rows;         // rows this context renders
    int32_t rank, world;        // 8-row strips s with s % world == rank
    int32_t max_bounces;        // main.glsl:377 literal 5 == max_bounces + 1
    int32_t accum_mode;         // JPT_ACCUM_*
    uint32_t frame_index;       // camera.frame_index of this frame (main.glsl:409)
    uint32_t frame_count;       // ProgressiveRendering frame_count of this frame (progressive_rendering.cpp:53-60)
    int32_t n_frames;           // frames rendered by one launch (wide kernels)
    int32_t depth_frame;        // launch-local index of the frame whose first-hit distance is the depth image (-1: none)
    int32_t display_mode;       // 0: screen = ACES of the running mean (progressive_rendering.glsl:39-45)
                                // 1: screen = the last frame's own rgba8 store (main.glsl:434), no pass after it
    int32_t debug_steps = 0;    // the shader's DEBUG_STEPS build (main.glsl:358-361,423-427): audit kernel only
};

// device view of ExactShadow (jpt_builder.h)
struct TieShadowDev {
    const RefBvhNode* __restrict__ bvh = nullptr;
    const RefTriGeometry* __restrict__ tri_geom = nullptr;   // reference order
    const RefInstance* __restrict__ instances = nullptr;
    const RefTlasNode* __restrict__ tlas = nullptr;
    const uint32_t* __restrict__ tri_native = nullptr;       // reference triangle -> native triangle
    const uint32_t* __restrict__ native_ref = nullptr;       // native triangle -> reference triangle
    const uint32_t* __restrict__ tri_leaf = nullptr;         // reference triangle -> its leaf node
    const uint32_t* __restrict__ subtree_end = nullptr;      // BVH node -> one past its subtree (pre-order numbering)
    const uint32_t* __restrict__ tlas_parent = nullptr;
    const uint32_t* __restrict__ inst_tlas_leaf = nullptr;
    bool ok = false;
    bool tlas_current = false;   // false after a device refit: `instances` and `tlas` are those of the last HOST update
};

// All device-resident scene data of a context.
struct DeviceScene {
    // reference layout (drop-in route + cold shading data)
    const RefTriGeometry* ref_tri_geom = nullptr;
    const ShadeTri* shade_tris = nullptr;   // (the 80-byte GpuTriangleData array itself stays on the host: jpt_scene_get_reference_buffer)
    const RefMaterial* ref_materials = nullptr;
    const RefBvhNode* ref_bvh = nullptr;
    const RefInstance* ref_instances = nullptr;
    const RefTlasNode* ref_tlas = nullptr;
    const uint8_t* tex = nullptr;
    uint32_t n_tris = 0, n_materials = 0, n_ref_bvh = 0, n_instances = 0, n_ref_tlas = 0;
    int32_t tex_res = 0, n_layers = 0;
    int32_t sampler_mode = 0;  // JPT_SAMPLER_* (jpt_set_params)
    // flattened layout (native route)
    const WideNode* blas_nodes = nullptr;
    const WideTri* wide_tris = nullptr;
    const WideNode* tlas_nodes = nullptr;
    const WideInstance* wide_instances = nullptr;
    int32_t tlas_root = 0;  // child reference of the TLAS root
    uint32_t n_blas_nodes = 0, n_tlas_nodes = 0;
    // four-child collapse of the same trees (native builder only; null otherwise)
    bool use4 = false;
    uint32_t stack_need4 = 0;                // worst-case pending entries of a walk over the four-child records (compute_stack_need)
    const WideNode4* nodes4 = nullptr;       // BLAS records followed by the TLAS records, one index space (float form: the
                                             // device refit of the TLAS works on these) ...
    const WideNodeQ* nodesq = nullptr;       // ... and their 64-byte quantised form, same indices: what the kernels walk
    const WideInstance* wide_instances4 = nullptr;
    int32_t tlas_root4 = 0;
    // reach records (jpt_types.h): null unless the scene was committed with JPT_BUILD_SAH
    const ReachTri* reach_tri = nullptr;
    const ReachInst* reach_inst = nullptr;
    // the reference's own trees beside a native scene (ExactShadow, jpt_builder.h): what wf2_finish decides exact distance
    // ties on (jpt_tie_walk.h).  x.ok false: not available (a watertight scene, uploaded trees that are not numbered in
    // pre-order) -- ties are then left to the order of the native walk.
    TieShadowDev x;

    SceneShading shading() const
    {
        SceneShading s;
        s.tri_data = shade_tris;
        s.instances = ref_instances;
        s.materials = ref_materials;
        s.tex = tex;
        s.n_materials = n_materials;
        s.n_instances = n_instances;
        s.sampler_mode = sampler_mode;
        s.reach_tri = reach_tri;
        s.reach_inst = reach_inst;
        s.retrace_ties = x.ok && reach_tri != nullptr;
        s.tex_res = tex_res;
        s.n_layers = n_layers;
        return s;
    }
};

#if defined(__HIPCC__)
// local row -> image row for the strip-interleaved partition
__device__ __forceinline__ int local_to_global_row(int ly, const FrameParams& fp)
{
    const int strip = ly / kStripRows;
    return (strip * fp.world + fp.rank) * kStripRows + (ly - strip * kStripRows);
}

// progressive_rendering.glsl:28-46 for one pixel, preceded by the rgba8 store of main.glsl:434 in
// REF_LDR8 mode.  accum: rgba32f frameBuffer; ldr: the rgba8 screen after ACES.
__device__ __forceinline__ void accumulate_pixel(const FrameParams& fp, size_t idx, f3 radiance, float4* __restrict__ accum,
                                                 uint32_t* __restrict__ ldr)
{
    f3 cur = radiance;
    if (fp.accum_mode == 0) {
        cur = mk3(from_unorm8(unorm8(radiance.x)), from_unorm8(unorm8(radiance.y)), from_unorm8(unorm8(radiance.z)));
    }
    f3 sum = cur;
    if (fp.frame_count > 1) {
        const float4 prev = accum[idx];
        sum = mk3(cur.x + prev.x, cur.y + prev.y, cur.z + prev.z);
    }
    accum[idx] = make_float4(sum.x, sum.y, sum.z, 1.0f);
    if (fp.display_mode == 1) {
        ldr[idx] = unorm8(radiance.x) | (unorm8(radiance.y) << 8) | (unorm8(radiance.z) << 16) | 0xFF000000u;
        return;
    }
    const float fc = (float)fp.frame_count;
    const f3 col = aces_film(mk3(sum.x / fc, sum.y / fc, sum.z / fc) * 1.0f);
    ldr[idx] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xFF000000u;
}

__device__ __forceinline__ void flush_counters(const DevCounters& c, DevCounters* __restrict__ out)
{
    if (c.rays) atomicAdd(&out->rays, c.rays);
    if (c.blas_expand) atomicAdd(&out->blas_expand, c.blas_expand);
    if (c.tri_tests) atomicAdd(&out->tri_tests, c.tri_tests);
    if (c.tlas_expand) atomicAdd(&out->tlas_expand, c.tlas_expand);
    if (c.inst_visits) atomicAdd(&out->inst_visits, c.inst_visits);
    if (c.shaded_hits) atomicAdd(&out->shaded_hits, c.shaded_hits);
    for (int k = 0; k < 8; k++)
        if (c.phase[k]) atomicAdd(&out->phase[k], c.phase[k]);
    if (c.walk_max) atomicMax(&out->walk_max, c.walk_max);
    for (int k = 0; k < 8; k++)
        if (c.walk_hist[k]) atomicAdd(&out->walk_hist[k], c.walk_hist[k]);
    if (c.zero_thr) atomicAdd(&out->zero_thr, c.zero_thr);
}
__device__ __forceinline__ void count_walk(DevCounters& c, uint32_t steps)
{
    if (steps > c.walk_max) c.walk_max = steps;
    int b = 0;
    for (uint32_t lim = 16u; b < 7 && steps >= lim; lim <<= 2) b++;
    c.walk_hist[b]++;
}
#endif

// the checks of jpt_set_environment / jpt_set_environment_params (jpt_lighting.cpp), also run by jpt_debug_env_lookup: JPT_OK, or a
// JPT_E_* code and the reason in `why`; and the map's device layout, (r, g, b, 0) per texel
int check_env_map(const float* rgb, int32_t width, int32_t height, std::string& why);
int check_env_params(const float* rotation9, float intensity, std::string& why);
void pack_env_texels(const float* rgb, int32_t width, int32_t height, std::vector<float4>& out);
// the checks of jpt_set_lens (jpt_primary.cpp), also run by jpt_debug_lens_rays
int check_lens(float aperture_radius, float focus_distance, std::string& why);
// the camera model of `model` seen through `cam` (jpt_primary.cpp; jpt_set_camera_model, also run by jpt_debug_camera_rays): the basis
// for EQUIRECT.  JPT_E_INVALID: no such model; JPT_E_STATE: EQUIRECT's basis or PROJECTIVE's ivp is not finite.
int make_camera_model(int32_t model, const RefCamera& cam, CamModelDev& out, std::string& why);
// the map's sampling tables built on the device (jpt_kernels_post.hip), on `stream`: cond (w * h floats), marg (h floats) and the
// total weight (one float), all device memory: one thread per row (env_build_row), then one thread for the marginal
void launch_env_tables(hipStream_t stream, const float4* texels, int32_t w, int32_t h, float* cond, float* marg, float* total);
// jpt_set_sky's launch (jpt_kernels_sky.hip), on `stream`: the w x h texels of `out` (16-byte aligned), (r, g, b, 0) each, from n x n
// subsamples of sky_radiance (jpt_sky.h).  Nothing else is written and nothing is read.  1 <= n <= kSkyMaxSamples; w, h within the map's limits.
void launch_sky(hipStream_t stream, const SkyDev& P, int32_t w, int32_t h, int32_t n, float4* out);
// the checks of jpt_set_sky (jpt_lighting.cpp), also run by the jpt_debug_sky entries, and what the kernel takes: JPT_OK and `out`, or a
// JPT_E_* code and the reason in `why`.  params NULL: the defaults.  The size and sample checks are sky_size_check's.
int sky_params_dev(const jpt_sky_params* params, SkyDev& out, std::string& why);
int sky_size_check(int32_t width, int32_t height, int32_t samples, std::string& why);
void jpt_sky_default_params(jpt_sky_params& out);
// the message jpt_debug_last_error returns (jpt_debug.hip), for the debug entries that live elsewhere
void set_debug_error(const std::string& why);
// JPT_ENV_SAMPLING_MIS needs an orthonormal rotation: every entry of R R^T within kEnvOrthoTol of the identity's
constexpr double kEnvOrthoTol = 1e-4;
bool env_rotation_orthonormal(const float* rotation9);

// What the misses and the shadow rays of one render see -- the whole answer, made once per render (resolve_lighting, jpt_lighting.cpp)
// and read by everything that sizes or launches it.  Host side only: the kernels take env, samp, lights and env_mode as they are.
struct Lighting {
    // the kernel family: the default kernels, *_env, *_mis, *_lt (emitter sampling over a scene with emitters, whatever the miss model)
    enum Kind { kSky, kMap, kMapMis, kEmitters } kind = kSky;
    int env_mode = 0;        // the miss model, a run-time value of the *_lt kernels: 0 the gradient, 1 the map, 2 the map with MIS
    EnvDev env = {};         // the map (env_mode != 0; zeroed otherwise)
    EnvSampDev samp = {};    // its sampling tables (env_mode == 2)
    LightDev lights = {};    // the emitter tables (kEmitters; zeroed otherwise: n == 0)
    // The scene has a transmissive material and the context reads the extension words (jpt_set_material_extensions): the launches
    // that shade take the general *_tx kernels instead of `kind`'s, with env_mode and `lights` as they are; the primary, trace,
    // occlude and accumulate launches stay those of `kind` and the miss model.
    bool transmissive = false;
    bool map_queues() const { return env_mode == 2; }           // the workspace holds the map's shadow queues (wf2_occlude) ...
    bool emitter_queues() const { return kind == kEmitters; }   // ... the emitters' (wf2_occlude_lt)
};

// Where the paths of one render start -- the whole answer, made once per render (resolve_primary, jpt_primary.cpp) and read by
// everything that prepares or launches it.  The members `kind` does not use are zeroed: radius 0, kCamPinhole, null images.  Host side
// only: the kernels take lens, cam_model, bake, probe and cube as they are.
struct PrimaryRays {
    // the pinhole; the thin lens (jpt_set_lens: the *_lens forms of the primary launch); a camera model other than the pinhole
    // (jpt_set_camera_model: the *_cam forms); the texel images (jpt_set_bake_texels: the *_bake forms); the probes (jpt_set_probes:
    // the *_probe forms); the reflection probes (jpt_set_reflection_probes: the *_cube forms)
    enum Kind { kPinhole, kLens, kCamModel, kBake, kProbe, kCube } kind = kPinhole;
    LensDev lens = {};
    CamModelDev cam_model = {};
    BakeDev bake = {};
    ProbeDev probe = {};
    CubeDev cube = {};
    // The sky cull, the tiles' sky cells and the cull window apply: the rectangles are the pinhole's projection of the boxes -- from a
    // point of the aperture a pixel outside them may still see geometry, another model projects otherwise, a bake's paths start on
    // the surfaces and a probe's (of either kind) at the probe.  False: Wf2Render::cull stays off (n < 0) and sky_tiles null.
    bool sky_cull() const { return kind == kPinhole; }
};

// one frame over the reference layout (jpt_kernels_ref.hip); counters may be null
void launch_ref_frame(hipStream_t stream, const DeviceScene& ds, const FrameParams& fp, const RefCamera& cam, float4* accum,
                      uint32_t* ldr, float* depth, DevCounters* counters, const Lighting& lg, const PrimaryRays& primary);

// The UV2 rasteriser of jpt_bake_add_surface (jpt_kernels_bake.hip), on `stream`: clears `winner` (width * height words), lets every
// triangle of `surf` claim the texels whose centres it covers (atomicMin of its index), then writes the texels that have a winner
// into position4 / normal4 (bake_resolve, jpt_bake.h) and leaves the others as they are.  Every pointer is device memory.
void launch_bake_raster(hipStream_t stream, const BakeSurfaceDev& surf, int32_t width, int32_t height, uint32_t* winner, float4* position4,
                        float4* normal4);
// the same on the host, over host memory: a plain loop over texels and triangles calling the same coverage and resolve functions
void bake_raster_host(const BakeSurfaceDev& surf, int32_t width, int32_t height, float4* position4, float4* normal4);
// the checks of jpt_set_bake_texels / jpt_bake_begin on the size (jpt_primary.cpp), also run by the jpt_debug_bake_* entry points
int check_bake_size(const char* call, int32_t width, int32_t height, std::string& why);
// ... of jpt_set_bake_texels on the images: a valid texel with a non-finite position or normal component is JPT_E_INVALID
int check_bake_texels(const char* call, const float* position4, const float* normal4, size_t n, std::string& why);
// ... and of jpt_bake_add_surface on the surface: null arrays, n_indices no multiple of 3, an index out of range (JPT_E_INVALID), more
// than 2^24 triangles (JPT_E_LIMIT)
int check_bake_surface(const char* call, const float* vertices, const float* normals, const int32_t* indices, int32_t n_vertices, int32_t n_indices,
                       const float* uv2, const float* transform12, std::string& why);

// jpt_set_probes / jpt_probe_project (jpt_probe.h).  The checks of jpt_set_probes (jpt_primary.cpp), also run by the jpt_debug_probe_*
// entry points: the tile and the counts, then (unless null) the positions.
int check_probes(const char* call, const float* position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row, std::string& why);
// the quadrature table of (tile_w, tile_h, flags): tile_w * tile_h * 9 floats, made in double (jpt_primary.cpp)
void probe_basis_table(int32_t tile_w, int32_t tile_h, int32_t flags, std::vector<float>& out);
// The projection (jpt_kernels_probe.hip), on `stream`: one wave per probe over the accumulation image (pd.per_row * pd.tile_w pixels
// wide; pd.position is not read), `table` as above, 9 float4 per probe into `out`.  Every pointer is device memory.
void launch_probe_project(hipStream_t stream, const ProbeDev& pd, const float4* accum, float frame_count, const float* table, float4* out);

// jpt_set_reflection_probes / jpt_reflection_prefilter (jpt_cube.h, jpt_reflection.h).  The checks of jpt_set_reflection_probes
// (jpt_primary.cpp), also run by the jpt_debug_cube_rays / jpt_debug_reflection_* entry points: the face size and the counts, then
// (unless null) the positions; and those of jpt_set_reflection_params against a face size (0: none known yet).
int check_reflection_probes(const char* call, const float* position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row, std::string& why);
int check_reflection_params(const char* call, int32_t n_levels, int32_t samples, int32_t face_size, std::string& why);
// The sample tables of (face_size, n_levels, samples), made in double (jpt_primary.cpp): n_levels * samples entries (L_x, L_y, L_z, w)
// and source levels, level l's at l * samples, the kept ones first and zeros / kReflNoSample behind them (level 0 has none);
// count[l]: how many are kept
void reflection_sample_table(int32_t face_size, int32_t n_levels, int32_t samples, std::vector<float4>& table, std::vector<uint8_t>& levels,
                             uint32_t count[kReflLevelsMax]);
// The two steps of jpt_reflection_prefilter (jpt_kernels_reflection.hip), on `stream`: the source chain of every probe from the
// accumulation image (rd.per_row * 6 * rd.face_size() pixels wide), then the output chain from it and the tables.  Every pointer is
// device memory; the layouts are jpt_reflection.h's.
void launch_reflection_chain(hipStream_t stream, const ReflDev& rd, const float4* accum, float frame_count, float4* chain);
void launch_reflection_prefilter(hipStream_t stream, const ReflDev& rd, const float4* chain, const float4* table, const uint8_t* levels, float4* out);

// The emitter tables (jpt_kernels_post.hip), on `stream`, from the scene's device arrays: cand holds n (instance, triangle) pairs;
// tri (3 n float4), cdf (n floats), marg (n_blocks + 1 floats: the marginal CDF, then the total power) are device memory
struct LightBuildArgs {
    const uint32_t* cand;
    uint32_t n, n_blocks;
    const RefInstance* instances;
    uint32_t n_instances, n_materials;
    const RefMaterial* materials;
    const WideTri* wtris;
    const ShadeTri* shade;
    float4* tri;
    float* cdf;
    float* marg;
};
void launch_light_tables(hipStream_t stream, const LightBuildArgs& a);
// the audit probe of jpt_debug_light_sample (what 1: xi4, origins) / jpt_debug_light_pdf (what 2: inst, tri, points, origins,
// dirs), device pointers, on `stream` (jpt_debug.hip)
void launch_light_probe(hipStream_t stream, const LightDev& lt, const SceneShading& sh, int what, const float* xi4, const float* origins,
                        const float* dirs, const float* points, const uint32_t* inst, const uint32_t* tri, uint32_t n, float* points_out,
                        float* dirs_out, float* pdf_out);

// The persistent-block pipeline (jpt_kernels_wf2.hip): one render of fp.n_frames frames over the flattened layout;
// fp.frame_index / fp.frame_count are those of the FIRST frame.  The first (max_bounces + 2) *
// wf2_segments() u32 of `workspace` are per-bounce, per-segment queue sizes afterwards; rows 1..max_bounces
// sum to the secondary ray segments traced.  trace_events: pairs around wf2_primary and each wf2_trace.
// The sky cell of every 8 x 8 tile of the context's share of the image whose four corner rays agree on one (wf2_sky_tiles: the
// tile-level test of wf2_accumulate, one lane per tile).  Depends on the camera, the image size and the partition only -- the host
// runs it when those change, not per render.  wf2_sky_tile_count: words `tile_cell` must hold.
size_t wf2_sky_tile_count(int width, int local_rows);
void launch_sky_tiles(hipStream_t stream, const FrameParams& fp, const RefCamera& cam, uint32_t* tile_cell);
uint32_t wf2_segments();
uint32_t trace_stack_capacity();  // entries a lane's traversal stack can hold (LDS + scratch)
// bytes of the workspace a render of this size carves (wf2_layout), for any frame-group count and window
size_t wf2_workspace_bytes(int width, int local_rows, int n_frames, int max_bounces, const Lighting& lg);   // lg: its shadow queues
// Screen rectangles (pixels, inclusive) of the boxes the TLAS root offers a ray; a primary ray through a pixel
// outside all of them is known to fail all of the root's box tests, i.e. to reach the sky after exactly one TLAS
// expansion, without being traced.  n < 0: unknown, trace everything.  Filled on the host (jpt_capi.cpp).
struct SkyCull {
    int32_t n = -1;
    int32_t x0[4], y0[4], x1[4], y1[4];
};

// what the context owns for running frame groups side by side: the helper stream of group k + 1 and the event group 0's stream
// waits on for it (launch_wf2_render uses the first groups - 1 of them)
struct Wf2Streams {
    hipStream_t aux_stream[kMaxGroups - 1] = {};
    hipEvent_t fork = nullptr, join[kMaxGroups - 1] = {};
};
// what one render passes to its launches
struct Wf2Render {
    SkyCull cull;                          // for the primary launch of this render
    hipEvent_t before_acc = nullptr;       // the accumulation kernel waits for this event (whatever its stream)
    const uint32_t* sky_tiles = nullptr;   // per 8 x 8 tile of the context's share of the image: its one rgba8 sky cell, if it has one
                                           // (launch_sky_tiles; null: wf2_accumulate decides every culled pixel by itself)
    Lighting lighting;                     // the kernel family of its launches and the workspace's shadow queues (no sky cells with a map)
    PrimaryRays primary;                   // which form of the primary launch it takes, and that form's argument
    float4* bake_dir = nullptr;            // jpt_set_bake_directional: the three moment planes a bake render adds to (launch_bake_moments
                                           // behind the accumulation); null: off, and no launch or argument differs
    float4* variance = nullptr;            // jpt_set_variance: the plane of second moments a render adds to (launch_variance_moments, jpt_variance.h,
                                           // in front of the accumulation; `cull` then stays off and `sky_tiles` null); null: off, likewise
};
// What the moment kernel of one bake render reads and writes (jpt_kernels_bake_dir.hip; the arithmetic: jpt_bake_dir.h): the
// per-(slot, frame) values wf2_accumulate reads, in its layout, and the three planes.  Every pointer is device memory.
struct BakeDirArgs {
    const float4* rad = nullptr;       // JPT_ACCUM_HDR_F32: the finished radiance per (slot, frame)
    const uint32_t* fin8 = nullptr;    // JPT_ACCUM_REF_LDR8: the same as rgba8 words
    const float4* normal = nullptr;    // the bake normal image, width x height (the whole image)
    float4* planes = nullptr;          // three planes of width x local_rows float4, plane k at k * width * local_rows
    int32_t full_tiles_x = 0, full_tiles_y = 0;   // the context's share of the image in 8 x 8 tiles: a bake render's window is all of it
    uint32_t slots_per_frame = 0;      // full_tiles_x * full_tiles_y * 64
    int32_t groups = 1;                // the frame groups whose blocks of rad / fin8 are read
};
// on `stream`: one thread per texel of the share; fp is the render's (frame_index / frame_count of its FIRST frame)
void launch_bake_moments(hipStream_t stream, const BakeDirArgs& a, const FrameParams& fp);
// `groups` frame groups (1..kMaxGroups, at most n_frames; groups > 1 needs streams.aux_stream[0 .. groups - 2]); `chain`: consecutive
// segments per tracing block
void launch_wf2_render(hipStream_t stream, const DeviceScene& ds, const FrameParams& fp, const RefCamera& cam, void* workspace,
                       float4* accum, uint32_t* ldr, float* depth, DevCounters* counters, hipEvent_t* trace_events,
                       const Wf2Render& r, int groups, int chain, const Wf2Streams& streams);

// one wave busy for `ticks` of the device's wall clock (hipDeviceAttributeWallClockRate), to see which streams run side by side
void launch_queue_spin(hipStream_t stream, long long ticks);

// Moving instances without the host (jpt_scene_refit_tlas, jpt_kernels_post.hip): instance records from new transforms, then the
// boxes of the four-child TLAS records bottom-up over the unchanged topology, then their quantised form.  Every pointer is a device
// pointer.
struct Tlas4RefitArgs {
    const float* transforms12 = nullptr;     // n_instances x 12 floats
    uint32_t n_instances = 0;
    const RefBvhNode* bvh = nullptr;         // the reference-layout BLAS nodes (root boxes)
    RefInstance* instances = nullptr;        // the copy of the instance level written
    WideInstance* wide_instances4 = nullptr;
    ReachInst* reach = nullptr;              // (may be null)
    const float* cut_boxes = nullptr;        // RefScene::inst_cut_boxes / inst_cut_range (may be null)
    const uint32_t* cut_range = nullptr;
    WideNode4* nodes4 = nullptr;
    WideNodeQ* nodesq = nullptr;
    uint32_t n_blas_records = 0;             // where the TLAS tail written starts in nodes4 / nodesq
    uint32_t n_tlas_records = 0;
    const uint32_t* order = nullptr;         // tlas4_refit_schedule
    const uint32_t* level_start = nullptr;
    uint32_t n_levels = 0;
    // before the boxes, the tail's topology (jpt_scene_rebuild_tlas, jpt_kernels_tlas.hip) -- made anew from the template's child words
    // (rebuild_child non-null: n_tlas_records x 4; sorted: n_instances words; sort_scratch: 2 n_instances keys, read beyond
    // kTlasLdsKeys instances only) -- or copied from the tail at copy_from (copy_tail: the copy written holds an older topology)
    const int32_t* rebuild_child = nullptr;
    uint32_t* sorted = nullptr;
    uint64_t* sort_scratch = nullptr;
    bool copy_tail = false;
    uint32_t copy_from = 0;
};
void launch_tlas4_refit(hipStream_t stream, const Tlas4RefitArgs& args);
// The steps of a rebuild alone (jpt_kernels_tlas.hip; every pointer a device pointer).  launch_tlas_order: boxes at lo / hi (`stride`
// floats between instances, n <= kTlasRebuildMaxInstances) -> the key of every instance (keys_out, may be null) and the instance at
// every position of the sorted order; one block.  launch_tlas_template: the template's child words into the records at `base`.
// launch_tlas_tail_copy: n_records records from one tail to another, internal references rebased.
void launch_tlas_order(hipStream_t stream, const float* lo, const float* hi, uint32_t stride, uint32_t n, uint64_t* keys_out, uint64_t* scratch,
                       uint32_t* sorted_out);
void launch_tlas_template(hipStream_t stream, const int32_t* tmpl, uint32_t n_records, const uint32_t* sorted, WideNode4* nodes4, uint32_t base);
void launch_tlas_tail_copy(hipStream_t stream, WideNode4* nodes4, uint32_t from_base, uint32_t to_base, uint32_t n_records);

// Deforming a committed mesh without the host (jpt_scene_update_mesh, jpt_kernels_mesh.hip): the mesh's triangle records from new
// vertices, its four-child BLAS records refitted bottom-up (order / level_start: refit4_schedule of the mesh, on the device;
// h_level_start: the same on the host, absolute indices into `order`), its root box in `bvh`, and the cut boxes of its instances
// dropped.  Every pointer is a device pointer.
struct MeshRefitArgs {
    const float* verts = nullptr;        // the mesh's vertices, surfaces end to end (3 floats each)
    const float* normals = nullptr;      // the same layout, or null: the vertex normals stay
    const uint32_t* vidx = nullptr;      // per triangle of the scene (device order): its three indices into verts
    uint32_t tri_first = 0, n_tris = 0;  // the mesh's triangles
    WideTri* wtris = nullptr;
    ShadeTri* shade = nullptr;
    int32_t* bounds = nullptr;           // 6 ordered keys (jpt_mesh_math.h): min xyz preset to +FLT_MAX, max xyz to -FLT_MAX
    WideNode4* nodes4 = nullptr;
    WideNodeQ* nodesq = nullptr;
    const uint32_t* order = nullptr;
    const uint32_t* level_start = nullptr;
    int32_t root4 = 0;                   // the mesh's root reference in nodes4 (a leaf reference when the mesh is one leaf)
    RefBvhNode* bvh = nullptr;
    uint32_t bvh_root = 0;               // the mesh's root in bvh (RefScene::mesh_roots)
    uint32_t* cut_range = nullptr;       // RefScene::inst_cut_range (may be null)
    const RefInstance* instances = nullptr;
    uint32_t n_instances = 0;
};
void launch_mesh_refit(hipStream_t stream, const MeshRefitArgs& args, const uint32_t* h_level_start, uint32_t n_levels);
// its two halves, for a caller that puts a new topology between them (jpt_scene_rebuild_mesh): the triangle records and the mesh's
// bounds; the records level by level, then the root box
void launch_mesh_tris(hipStream_t stream, const MeshRefitArgs& args);
void launch_mesh_records(hipStream_t stream, const MeshRefitArgs& args, const uint32_t* h_level_start, uint32_t n_levels);

// A new topology for a committed mesh (jpt_scene_rebuild_mesh, jpt_kernels_mesh_rebuild.hip; the arithmetic: jpt_mesh_rebuild.h): the
// mesh's triangles in ascending (Morton code of the vertex box's centre, triangle) order.  `work`: mesh_sort_words(n_tris) words of
// device memory, written and read by these launches only.  launch_mesh_order_codes: the bounds of the centres, then at mesh_order_codes
// the code of every triangle and at mesh_order_sorted tri_first + its index in the mesh, both in triangle order (jpt_debug_mesh_order
// copies the codes out here); launch_mesh_order_sort: both arrays sorted in place (through the second pair of buffers and back), so
// mesh_order_sorted holds the triangle at every sorted position; launch_mesh_order: all of it.
struct MeshOrderArgs {
    const float* verts = nullptr;      // as MeshRefitArgs
    const uint32_t* vidx = nullptr;
    uint32_t tri_first = 0, n_tris = 0;
    uint32_t* work = nullptr;
};
inline uint32_t* mesh_order_codes(const MeshOrderArgs& a) { return a.work + 8; }
inline uint32_t* mesh_order_sorted(const MeshOrderArgs& a) { return a.work + 8 + a.n_tris; }
void launch_mesh_order_codes(hipStream_t stream, const MeshOrderArgs& args);
void launch_mesh_order_sort(hipStream_t stream, const MeshOrderArgs& args);
inline void launch_mesh_order(hipStream_t stream, const MeshOrderArgs& args)
{
    launch_mesh_order_codes(stream, args);
    launch_mesh_order_sort(stream, args);
}
// the root word of every instance of the mesh at `bvh_root` in one copy of the instance level (instance_refit_kernel never writes it)
void launch_mesh_root_words(hipStream_t stream, WideInstance* winst4, const RefInstance* instances, uint32_t n_instances, uint32_t bvh_root, int32_t root);

// Posing a committed mesh on the device (jpt_scene_pose_mesh, jpt_kernels_skin.hip; the arithmetic: jpt_skin.h): one thread per vertex
// of the mesh writes packed float3 positions -- and normals, when the rig has them -- where the mesh refit reads them
// (MeshRefitArgs::verts / normals); the lanes gather their bones from the palette in global memory.  Every pointer is a device pointer, 16-byte aligned; no bone index of the rig
// may reach n_bones (the host checks: check_skin_pose).
struct SkinArgs {
    SkinRig rig;
    int32_t influences = 0;               // 0, 4 or 8
    const float* palette = nullptr;       // n_bones x 12 floats (transform12 layout)
    uint32_t n_bones = 0;
    const SkinShape* active = nullptr;    // the pose's shapes with a weight != 0, ascending
    uint32_t n_active = 0;
    float* verts_out = nullptr;
    float* normals_out = nullptr;         // written when rig.bind_nrm is set
};
void launch_mesh_skin(hipStream_t stream, const SkinArgs& args);
// The host halves, shared by the context calls and jpt_debug_skin.  A rig arrives as pieces (one per surface, host pointers, vertices end
// to end); check_skin_rig runs jpt_scene_set_mesh_rig's argument checks on them (`with_normals`: the bind pose carries normals) and lays
// the rig out as one block of `bytes`; pack_skin_rig fills such a block (bone indices to 16 bits, deltas shape-major over the whole
// mesh); skin_rig_view points into a block at `base` (host or device).  check_skin_pose runs jpt_scene_pose_mesh's checks and compacts
// the blend weights into the active list.
struct SkinPiece {
    int32_t n_vertices = 0;
    const float* positions = nullptr;
    const float* normals = nullptr;
    const int32_t* bones = nullptr;
    const float* weights = nullptr;
    const float* dpos = nullptr;
    const float* dnrm = nullptr;
};
struct SkinRigInfo {
    uint32_t n_vertices = 0;
    int32_t influences = 0, n_shapes = 0;
    int32_t max_bone = -1;                // the largest bone index the rig names (-1: none)
    bool with_normals = false, with_dnrm = false;
    size_t off_pos = 0, off_nrm = 0, off_bones = 0, off_weights = 0, off_dpos = 0, off_dnrm = 0, bytes = 0;
};
int check_skin_rig(const char* call, const SkinPiece* pieces, int32_t n_pieces, int32_t influences, int32_t n_shapes, bool with_normals,
                   SkinRigInfo& info, std::string& why);
void pack_skin_rig(const SkinRigInfo& info, const SkinPiece* pieces, int32_t n_pieces, char* out);
SkinRig skin_rig_view(const SkinRigInfo& info, const char* base);
int check_skin_pose(const char* call, const SkinRigInfo& info, const float* bone_transforms12, uint32_t n_bones, const float* blend_weights,
                    uint32_t n_blend_weights, std::vector<SkinShape>& active, std::string& why);

// one dispatch of temporal_reprojection.glsl over a whole image (jpt_kernels_post.hip): screen rgba8 in/out, depth
// read-only, hist1 / hist2 the two rgba32f history images
void launch_temporal(hipStream_t stream, const RefTemporalParams& tp, uint32_t* screen, const float* depth, float4* hist1,
                     float4* hist2);

// jpt_denoise (jpt_kernels_denoise.hip; the arithmetic: jpt_denoise.h).  The checks of jpt_set_denoise_params, also run by
// jpt_debug_atrous; the guide images of the whole image -- one primary ray per pixel through the pixel centre over the arrays the
// wavefront kernels walk, (position.xyz, hit distance | -1), (normal, 0), (albedo, 0) per pixel --; and the filter passes: from the
// sums and frame_count to the denoised image in `ping` ((r, g, b, 1); `pong` is scratch) and its display image in `ldr` (may be
// null).  Every pointer is a device pointer of width * height elements; nothing else is written.
struct AtrousParams;
int check_denoise_params(const AtrousParams& p, std::string& why);
void launch_guides(hipStream_t stream, const DeviceScene& ds, const RefCamera& cam, const CamModelDev& cm, int width, int height,
                   float4* position_t, float4* normal, float4* albedo);
void launch_atrous(hipStream_t stream, const AtrousParams& prm, int width, int height, const float4* sums, float frame_count,
                   const float4* position_t, const float4* normal, const float4* albedo, float4* ping, float4* pong, uint32_t* ldr);
// jpt_denoise with jpt_set_denoise_variance on (jpt_kernels_denoise_var.hip; the arithmetic: jpt_denoise_var.h): launch_atrous' passes
// with the colour weight measured against the variance of the mean, from pass `first_pass` on, which reads `src` -- pass 0: the sums, and
// with them `m2`, the plane of jpt_set_variance, of frame_count >= 2 frames; a later pass: an (i, v) image (neither `ping` nor `pong` when
// passes - first_pass is even), m2 and frame_count not read.  Also writes `var_out`, width * height floats: the variance the last pass
// leaves.  sigma_color is not read.
struct AtrousVarParams;
void launch_atrous_variance(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, int first_pass, const float4* src,
                            const float4* m2, uint32_t frame_count, const float4* position_t, const float4* normal, const float4* albedo, float4* ping,
                            float4* pong, uint32_t* ldr, float* var_out);
// jpt_denoise with jpt_set_denoise_history on (jpt_kernels_denoise_history.hip; the arithmetic: jpt_denoise_history.h).  The stage: from
// the sums, frame_count, this call's guides and the previous history set (three planes, or three nulls) seen from `prev_view` (not read
// with `same_view`) to the new set and the (m, v_0) image `iv`; and the filter over `iv`: a first pass of its own, then
// launch_atrous_variance from pass 1 -- outputs as launch_atrous_variance's.  `iv` is neither `ping` nor `pong`.
struct HistoryParams;
struct HistoryView;
void launch_denoise_history(hipStream_t stream, const HistoryParams& hp, int normal_power_log2, int width, int height, const float4* sums, uint32_t frame_count,
                            const float4* position_t, const float4* normal, const float4* albedo, const HistoryView& prev_view, bool same_view,
                            const float4* prev_a, const float4* prev_b, const float4* prev_x, float4* new_a, float4* new_b, float4* new_x, float4* iv);
void launch_atrous_history(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, const float4* iv,
                           const float4* position_t, const float4* normal, const float4* albedo, float4* ping, float4* pong, uint32_t* ldr, float* var_out);

// jpt_bake_finish (jpt_kernels_lightmap.hip; the arithmetic: jpt_lightmap.h).  The checks of jpt_set_bake_finish_params, also run by
// jpt_debug_bake_finish; and the whole transform on `stream`: the guides (xg, ng) from the bake images, `passes` filter passes from
// the sums and frame_count, `dilate` dilation passes -- ping-pong between `ping` and `pong`; the one that holds the lightmap ((r, g,
// b, coverage) per texel) is returned.  Every pointer is a device pointer of width * height elements; nothing else is written.
struct LightmapParams;
int check_bake_finish_params(const char* call, const LightmapParams& p, std::string& why);
float4* launch_lightmap_finish(hipStream_t stream, const LightmapParams& prm, int width, int height, const float4* sums, float frame_count,
                               const float4* position4, const float4* normal4, float4* xg, float4* ng, float4* ping, float4* pong);

// jpt_query_rays / jpt_query_pixels (jpt_kernels_query.hip): n jpt_ray records walked over the arrays the wavefront kernels walk,
// one lane per ray; closest: a jpt_ray_hit per ray into `hits` and, unless null, a byte per ray into `occluded`; any: the byte alone
// (`hits` is not touched).  And the rays of n raster positions (x, y pairs) from the camera, as jpt_query_pixels forms them.  Every
// pointer is a device pointer, 16-byte aligned.
void launch_query(hipStream_t stream, const DeviceScene& ds, bool any, const void* rays, uint32_t n, void* hits, void* occluded);
void launch_query_pixel_rays(hipStream_t stream, const RefCamera& cam, const CamModelDev& cm, int width, int height, const void* xy, uint32_t n,
                             void* rays);

// pixels of this context's share of the image that lie outside the render's window (the tile-aligned bounding rectangle
// of the sky cull's screen rectangles): the primary launch does not even enumerate them (their rays are sky by the
// cull's argument; the event counters are completed with their number on the host)
uint64_t wf2_pixels_outside_window(const SkyCull& cull, const FrameParams& fp);

// rank-major gathered strips -> full framebuffer (multi-GPU assemble); the rows of `own_rank`, the gathering rank itself, are
// read from `own` (its local buffer), not from the gathered pieces
void launch_assemble(hipStream_t stream, const float4* gathered, const float4* own, int own_rank, int world, int width, int height,
                     int max_local_rows, float4* accum_full, uint32_t* ldr_full, uint32_t frame_count);

// the display image alone (each rank has already tone-mapped its own rows)
void launch_assemble_ldr(hipStream_t stream, const uint32_t* gathered, const uint32_t* own, int own_rank, int world, int width,
                         int height, int max_local_rows, uint32_t* ldr_full);

}  // namespace jpt
