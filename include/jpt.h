/*
 * jpt.h -- C ABI of libjpt_hip.so, the MI355X (gfx950) back end for the GDPathTracing hot path.
 *
 * This is the drop-in boundary.  In the reference the path sits behind the
 * `gdcs::ComputeShader` object (absent submodule src/gdcs) that PathTracingCamera and
 * ProgressiveRendering drive, plus the CPU builder in src/bvh that GeometryGroup3D::build calls.
 * Each entry point below names the reference call(s) it replaces (paths relative to the reference
 * repository).  Plain pointers and sizes only; caller-owned host memory, library-owned device memory;
 * every function returns 0 on success or a negative JPT_E_* code and records a message readable with
 * jpt_last_error().  One context per GPU and per host thread; calls are blocking unless noted.
 *
 * All matrices are column-major float[16] as src/utils.h:15-49 writes them; all structs are the
 * little-endian wire formats of SURVEY.md 8(a) T-3..T-11 (gdpathtracing_amd/csrc/jpt_types.h).
 */
#ifndef JPT_H
#define JPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPT_ABI_VERSION 6

typedef struct jpt_ctx jpt_ctx;

enum {
    JPT_OK = 0,
    JPT_E_INVALID = -1,      /* bad argument / call order */
    JPT_E_DEVICE = -2,       /* HIP error (no GPU, launch failure, out of memory) */
    JPT_E_LIMIT = -3,        /* scene exceeds a format limit (e.g. 16-bit TLAS child index, bvh.h:59) */
    JPT_E_STATE = -4         /* scene / params / camera not set */
};

/* accumulation modes */
enum {
    JPT_ACCUM_REF_LDR8 = 0,  /* per frame: clamp01 + 8-bit quantise, then float sum (what the reference does:
                                main.glsl:98,434 -> progressive_rendering.glsl:33-37) */
    JPT_ACCUM_HDR_F32 = 1    /* pure float sum of radiance */
};

/* Sampler of texture(textureArray, vec3(uv, layer)) (main.glsl:213-214).  The reference sets the sampler state inside
 * the absent gdcs (format set up at path_tracing_camera.cpp:178-184), so it is a parameter here;
 * bit 0 = repeat instead of clamp-to-edge, bit 1 = linear instead of nearest.  What each mode computes is pinned in
 * oracle/oracle_trace.c::sample_texture (Vulkan texel addressing, UNORM8 texels, no sRGB decode, no mipmaps:
 * geometry_group3d.cpp:294-300). */
enum {
    JPT_SAMPLER_NEAREST_CLAMP = 0,   /* default: Godot's RDSamplerState defaults */
    JPT_SAMPLER_NEAREST_REPEAT = 1,
    JPT_SAMPLER_LINEAR_CLAMP = 2,
    JPT_SAMPLER_LINEAR_REPEAT = 3
};

/* post-processing after the path-tracing pass: PathTracingCamera::Denoising (path_tracing_camera.h:30-34,
 * the switch at path_tracing_camera.cpp:207-225) */
enum {
    JPT_DENOISE_PROGRESSIVE = 0, /* ProgressiveRendering: running sum, screen = ACES(mean) (progressive_rendering.glsl) */
    JPT_DENOISE_TEMPORAL = 1,    /* TemporalReprojection: blend with the reprojected history (temporal_reprojection.glsl) */
    JPT_DENOISE_NONE = 2         /* nothing: the screen is main.glsl's own rgba8 store (main.glsl:434) */
};

/* BVH builders */
enum {
    JPT_BUILD_REFERENCE_EXACT = 0, /* reproduces src/bvh/bvh.cpp node-for-node (incl. its default-box quirk);
                                      kernels traverse the same tree in the same order */
    JPT_BUILD_SAH = 1,             /* native binned-SAH builder, flattened wide-fetch layout (fast path).  Also runs the
                                      reference's builder once per mesh to record which leaf box holds each triangle
                                      ("reach records"): a hit found on the native tree is checked against the two box
                                      tests that decide whether the reference's traversal reaches that triangle at all
                                      (main.glsl:259-350), so the image equals the reference's even where float rounding
                                      lets a reference ray slip through its own boxes.  The reference's
                                      trees are kept beside the native ones: a hit that ties with another at exactly the
                                      same distance -- whose winner is a matter of the reference's visiting order,
                                      main.glsl:247 -- is decided by the reference's own walk */
    JPT_BUILD_SAH_WATERTIGHT = 2   /* the native builder alone (half the build time): every triangle hit is found; differs
                                      from the reference's image in the few pixels per 10^7 paths where the reference's
                                      tree has such a crack */
};

/* which reference-layout buffer (GeometryGroup3D::get_*_buffer, geometry_group3d.cpp:40-68) */
enum {
    JPT_BUF_TRI_GEOMETRY = 0, /* GpuTriangleGeometry[]  48 B */
    JPT_BUF_TRI_DATA = 1,     /* GpuTriangleData[]      80 B */
    JPT_BUF_MATERIALS = 2,    /* GpuMaterial[]          64 B */
    JPT_BUF_BVH_NODES = 3,    /* BVH::BVHNode[]         48 B */
    JPT_BUF_INSTANCES = 4,    /* BVH::BLASInstance[]   176 B */
    JPT_BUF_TLAS_NODES = 5,   /* BVH::TLASNode[]        32 B */
    JPT_BUF_TRIANGLES = 6,    /* BVH::Triangle[]       144 B (builder-internal, bvh.h:22-29) */
    /* not reference buffers -- the reach records of a native-tree scene (csrc/jpt_types.h), for tests and audits: */
    JPT_BUF_REACH_TRIANGLES = 7, /* 32 B per triangle (JPT_BUF_TRI_GEOMETRY order): lo.xyz, always, hi.xyz, pad */
    JPT_BUF_REACH_INSTANCES = 8  /* 64 B per instance: world box lo.xyz _ hi.xyz _, reference root box lo.xyz _ hi.xyz _ */
};

/* One ArrayMesh surface as BVHBuilder::BuildBVH reads it (bvh.cpp:192-198). */
typedef struct {
    const float   *vertices;   /* n_vertices * 3   Mesh::ARRAY_VERTEX  */
    const float   *normals;    /* n_vertices * 3   Mesh::ARRAY_NORMAL  */
    const float   *uvs;        /* n_vertices * 2   Mesh::ARRAY_TEX_UV  */
    const int32_t *indices;    /* n_indices        Mesh::ARRAY_INDEX   */
    int32_t n_vertices;
    int32_t n_indices;
} jpt_surface;

typedef struct {
    uint64_t rays;             /* ray segments traced = ray_trace() invocations (main.glsl:352) */
    uint64_t frames;           /* frames rendered since jpt_accum_reset */
    uint64_t blas_expand;      /* node expansions / tests, only filled by counting renders (jpt_render_counted) */
    uint64_t tri_tests;
    uint64_t tlas_expand;
    uint64_t inst_visits;
    uint64_t shaded_hits;
    double   last_render_ms;   /* device time of the last jpt_render (HIP events on the ctx stream) */
    double   last_trace_ms;    /* of which: the path-tracing kernel(s) */
    double   last_build_ms;    /* host time of the last scene commit (builder + flatten + upload) */
    uint64_t phase[8];         /* counting renders: wave-level phase statistics of the tracing kernels (diagnostic) */
    uint64_t sky_culled;       /* counting renders: primary rays finished without a walk (their pixel lies outside the screen
                                  rectangles of the TLAS root's boxes); they ARE counted in `rays` and `tlas_expand`, as the
                                  reference expands the root for them, but no record is fetched */
    double   last_primary_ms;  /* kernel timing on: the bounce-0 launch alone (last_trace_ms = all traversal launches) */
    uint64_t set_aside;        /* blocking renders on a native tree with reach records: path vertices whose hit is undecidable on
                                  the native tree -- the reference's traversal cannot reach it (a crack of its boxes), or
                                  another triangle lies at exactly the same distance --, traced again on the reference's own
                                  trees after the last bounce */
    uint64_t set_aside_dropped;/* ... of which: more than the set-aside buffer holds (1/64 of the paths, at least 65 536) -- those
                                  were shaded as found (the native tree's closest hit: the image differs from the reference's
                                  in those pixels).  0 on every scene measured; a scene that reports more renders exactly with
                                  JPT_KERNEL_REFERENCE_LAYOUT or JPT_UPLOAD_WALK_AS_GIVEN / JPT_BUILD_REFERENCE_EXACT */
    /* ABI 4 -- counting renders with the wavefront kernels: how long the walks are.  A launch cannot end before its longest
     * ray does, one dependent fetch after another (launch tails). */
    uint64_t walk_steps_max;    /* most record steps (internal records + leaf turns + instance entries) one ray took */
    uint64_t walk_steps_hist[8];/* rays that took < 16, < 64, < 256, < 1024, < 4096, < 16384, < 65536, more steps */
    /* ABI 5 -- counting renders: path vertices that go on although their throughput has become exactly (0, 0, 0) (brdf()
     * returns 0 when n.v < 0, brdfs.glsl:14): every later vertex of such a path adds 0 * emission (main.glsl:380), SURVEY.md
     * section 7 lists ending them as a result-preserving freedom; DESIGN.md section 8 says what share of the rays they are */
    uint64_t zero_throughput;   /* ... such vertices (each is the start of one more ray segment) */
} jpt_stats;

/* ---- lifetime --------------------------------------------------------------------------------- */

/* replaces: RenderingServer::create_local_rendering_device() + new ComputeShader(...)
 * (path_tracing_camera.cpp:114,139; progressive_rendering.cpp:25).
 * device_id = JPT_DEVICE_HOST_ONLY makes a builder-only context: the jpt_scene_* calls and
 * jpt_scene_get_reference_buffer work without a GPU; everything that renders returns JPT_E_DEVICE
 * (there is no CPU fallback). */
#define JPT_DEVICE_HOST_ONLY (-1)
int jpt_create(int device_id, jpt_ctx **out);
void jpt_destroy(jpt_ctx *ctx);
const char *jpt_last_error(const jpt_ctx *ctx);   /* ctx may be NULL: error of the last failed jpt_create */
int jpt_abi_version(void);

/* Run all work of this ctx on an existing HIP stream (hipStream_t as void*), e.g. torch's current
 * stream.  NULL restores the context's own stream.  Work already queued on the previous stream is waited for.
 * No reference counterpart. */
int jpt_set_stream(jpt_ctx *ctx, void *hip_stream);
/* The stream this ctx orders its work on (its own one unless jpt_set_stream replaced it), as hipStream_t: lets a
 * framework queue its own work -- a collective on the finished rows -- behind the renders (bench.py wraps it in
 * torch.cuda.ExternalStream).  No reference counterpart. */
int jpt_get_stream(jpt_ctx *ctx, void **hip_stream);
/* Queued renders (jpt_render_async) run their path kernels on four or six internal streams ("pipeline slots").  The HIP
 * runtime deals the streams of a process onto a small pool of hardware queues PER PRIORITY LEVEL, and streams that share
 * a queue run in submission order; so by default the slots are created at the device's HIGHEST stream priority, whose
 * pool they have to themselves as long as the host, torch and RCCL keep their streams at the normal level (DESIGN.md
 * section 4: C3 1.05 ms per queued render against 1.34 with everything at the normal level).  That choice also lets the
 * slots pre-empt the host's own compute work on a shared device.  An embedding application that wants otherwise says so
 * per context, before its first queued render or at any later time (existing slot streams are drained and re-made):
 *   DEFAULT  the library's rule (highest level)
 *   NORMAL   the level everything else uses: no pre-emption of host work; the queued rate then depends on which streams
 *            happen to share a hardware queue
 *   HIGH / LOW   the device's highest / lowest level
 * The pool has GPU_MAX_HW_QUEUES queues per level -- four unless the environment says otherwise at the process's FIRST HIP call.
 * Six renders in flight are worth 4 % on a 1920x1080x8-spp render and 15 % on small ones when the slots' six streams get a queue
 * each, and cost as much when they have to share four.  PROCESS ENVIRONMENT: the library never writes it (a setenv from a
 * shared library races with every getenv of a multi-threaded host and changes the queue count for all other HIP users of the
 * process).  A host that wants six renders in flight exports a pool of six queues per level (GPU_MAX_HW_QUEUES) itself, before its
 * first HIP call and before it starts threads (bench.py and the Python binding leave it to their caller; six, not more: with eight
 * a SECOND context's streams pair up on some queues and it renders a third slower).  Every context MEASURES, before its first queued
 * render, whether six of its streams run side by side (~1 ms) -- six slots if they do, four if not: a host that exports nothing
 * gets four, which is also all that one blocking render per displayed frame (the addon's use) can ever use.
 * jpt_renders_in_flight: the slots the last queued render was dealt among (0 before the first).
 * No reference counterpart. */
enum { JPT_STREAM_PRIORITY_DEFAULT = 0, JPT_STREAM_PRIORITY_NORMAL = 1, JPT_STREAM_PRIORITY_HIGH = 2, JPT_STREAM_PRIORITY_LOW = 3 };
int jpt_set_stream_priority(jpt_ctx *ctx, int32_t priority);
int jpt_renders_in_flight(const jpt_ctx *ctx);

/* Device memory a context may spend on renders in flight.  A wavefront render keeps 168 bytes per path (pixel x frame of
 * the render window) in a workspace, and queued renders (jpt_render_async) use four or six workspaces at once -- 11 GB for
 * four 1920x1080x8-spp renders: fine on a 288 GB device the library has to itself, the first thing an application sharing
 * the GPU with its own renderer will want to cap.
 *   renders_in_flight  1..8 workspaces / pipeline slots; 0: the library's rule (4, or 6 where six slot streams run side by side;
 *                      2 when one workspace exceeds 24 GiB).
 *                      1 serialises queued renders (about 1.5 x the time per render at C3's size).
 *   workspace_budget_bytes  most bytes ONE workspace may take; a render with more frames than fit runs as batches of
 *                      frames in frame order, same image (0: the library's rule, 24 GiB).  One frame is the smallest
 *                      batch: when a single frame of the current resolution does not fit a budget set here, the
 *                      render calls return JPT_E_LIMIT and allocate nothing (the audit kernel needs no workspace).
 * Takes effect with the next render; workspaces no longer allowed are freed at once (the call waits for renders in
 * flight).  jpt_get_workspace_bytes reports what is allocated now.  No reference counterpart (the reference's
 * workspace is the two images of one frame).
 * Host side: the blocking read-backs (jpt_read_*) go through one PINNED staging buffer per context, as large as the
 * largest read-back made so far (133 MB after a jpt_read_accum_f32 of a 3840x2160 image); this call and every change of
 * resolution or partition give it back, the next read-back allocates what it needs.  It is not part of the bytes reported.
 * Nor are jpt_denoise's own images (84 bytes per pixel, from the first jpt_denoise at a resolution until jpt_set_params with
 * another size or jpt_destroy), nor jpt_display's (25.4 bytes per pixel, likewise), nor jpt_bake_finish's (64 bytes per texel):
 * jpt_get_workspace_bytes keeps reporting the renders' workspaces alone. */
int jpt_set_memory_policy(jpt_ctx *ctx, int32_t renders_in_flight, uint64_t workspace_budget_bytes);
int jpt_get_workspace_bytes(jpt_ctx *ctx, uint64_t *bytes_out);

/* ---- scene ingest, route (i): reference layout ------------------------------------------------ */

/* replaces: the six cs->create_storage_buffer_uniform(geometry_group->get_*_buffer(), b, 1) calls and
 * cs->create_layered_image_uniform(textures, ...) (path_tracing_camera.cpp:170-175,178-184).  Buffers are
 * byte-for-byte what GeometryGroup3D emits (geometry_group3d.cpp:40-68).  tex_rgba8 may be NULL.
 * What the kernels then walk is the library's NATIVE tree (four-child quantised records built over the uploaded
 * triangles of every BLAS an instance names), and the uploaded boxes that decide what the reference's traversal can reach
 * -- each triangle's BVHNode leaf (tri_count > 0), each instance's TLAS leaf -- become the reach records that keep the
 * image the reference's (see JPT_BUILD_SAH): the addon keeps GeometryGroup3D::build() and renders at the native route's
 * rate; the uploaded trees themselves are kept on the device too, and decide exact distance ties (see JPT_BUILD_SAH).
 * No builder of the reference is re-run.  Arrays that are not such a tree (a node or triangle reachable twice,
 * boxes that are not nested, an instance in no / several TLAS leaves, transform and inverse_transform that do not belong
 * together) are walked node for node as uploaded, like JPT_UPLOAD_WALK_AS_GIVEN; jpt_scene_upload_note says why.
 * After a native upload jpt_scene_get_reference_buffer returns the native trees in reference layout (triangles in the
 * native order), not the caller's arrays. */
int jpt_scene_upload_reference_layout(jpt_ctx *ctx,
                                      const void *tri_geometry, uint32_t n_triangles,
                                      const void *tri_data,
                                      const void *materials, uint32_t n_materials,
                                      const void *bvh_nodes, uint32_t n_bvh_nodes,
                                      const void *blas_instances, uint32_t n_instances,
                                      const void *tlas_nodes, uint32_t n_tlas_nodes,
                                      const uint8_t *tex_rgba8, int32_t tex_res, int32_t n_layers);

/* How the next jpt_scene_upload_reference_layout treats the trees it is given (no reference counterpart). */
enum {
    JPT_UPLOAD_NATIVE_TREE = 0,   /* default: native tree + reach records from the uploaded leaf / instance boxes */
    JPT_UPLOAD_WALK_AS_GIVEN = 1  /* audit route: the uploaded BVHNode / TLASNode arrays are walked node for node, in the
                                     reference's visit order (the six event counters equal the reference's too);
                                     ~20x slower on the demo scene, whose reference boxes are inflated to the origin */
};
int jpt_set_upload_mode(jpt_ctx *ctx, int32_t mode);
/* Which tree the kernels walk for the scene this context holds (>= 0), or a negative JPT_E_* code. */
enum {
    JPT_TREE_NONE = 0,              /* no scene */
    JPT_TREE_AS_GIVEN = 1,          /* uploaded reference-layout arrays, node for node */
    JPT_TREE_REFERENCE_EXACT = 2,   /* JPT_BUILD_REFERENCE_EXACT commit */
    JPT_TREE_NATIVE_REACH = 3,      /* native tree + reach records (JPT_BUILD_SAH commit, or a native upload) */
    JPT_TREE_NATIVE_WATERTIGHT = 4  /* JPT_BUILD_SAH_WATERTIGHT commit */
};
int jpt_scene_tree_kind(jpt_ctx *ctx);
/* Empty unless the last jpt_scene_upload_reference_layout is walked as given: then the reason. */
const char *jpt_scene_upload_note(const jpt_ctx *ctx);
/* 1: hits at exactly equal distance -- whose winner is a matter of the reference's visiting order, main.glsl:247 -- are
 * decided as the reference decides them for the scene this context holds (by the reference's own walk of the trees kept
 * beside the native ones; trivially on JPT_TREE_AS_GIVEN / JPT_TREE_REFERENCE_EXACT trees).  0: they fall to the native
 * tree's order, and *why_out (may be NULL; valid until the next scene call) says why: a JPT_BUILD_SAH_WATERTIGHT commit, or
 * an upload whose BLAS nodes are not numbered in pre-order (left child = parent + 1, as bvh.cpp:108-185 numbers them), which
 * the restricted walk needs -- such an upload still renders on the native tree with reach records; only the winners of exact
 * ties may differ from the reference's.  jpt_stats.set_aside keeps counting the tied vertices either way.  Negative: JPT_E_*. */
int jpt_scene_ties_exact(jpt_ctx *ctx, const char **why_out);

/* ---- scene ingest, route (ii): native build --------------------------------------------------- */

/* replaces GeometryGroup3D::build's tail (geometry_group3d.cpp:305-365): */
int jpt_scene_begin(jpt_ctx *ctx);
/*   BVHBuilder::BuildBVH(bvh_nodes, triangles, mesh)                 geometry_group3d.cpp:311, bvh.cpp:187-223 */
int jpt_scene_add_mesh(jpt_ctx *ctx, const jpt_surface *surfaces, int32_t n_surfaces, uint32_t *mesh_id_out);
/*   BLASInstance::{set_materials,set_transform}                      geometry_group3d.cpp:328-333, bvh.h:73-115
 *   transform12 = godot Transform3D: basis rows (xx xy xz yx yy yz zx zy zz) then origin (x y z). */
int jpt_scene_add_instance(jpt_ctx *ctx, uint32_t mesh_id, const float *transform12,
                           const int32_t *material_ids, int32_t n_material_ids);
/*   materials.push_back(gpu_material) / textures                     geometry_group3d.cpp:271-304 */
int jpt_scene_set_materials(jpt_ctx *ctx, const void *materials, uint32_t n_materials);
int jpt_scene_set_textures(jpt_ctx *ctx, const uint8_t *tex_rgba8, int32_t tex_res, int32_t n_layers);
/*   TLAS::build + Triangle -> GpuTriangle split + upload             geometry_group3d.cpp:350-365 */
int jpt_scene_commit(jpt_ctx *ctx, int32_t builder);
/* GeometryGroup3D::get_*_buffer() (geometry_group3d.cpp:40-68): valid after a REFERENCE_EXACT commit.
 * out may be NULL to query the size. */
int jpt_scene_get_reference_buffer(jpt_ctx *ctx, int32_t which, void *out, size_t capacity, size_t *size_out);

/* The committed scene of `src` (either route) made the scene of `dst` as well -- another context, normally on another
 * GPU: host arrays are copied and uploaded to dst's device, no builder runs again.  For one scene on several GPUs. */
int jpt_scene_share(jpt_ctx *dst, jpt_ctx *src);

/* ---- moving instances ---------------------------------------------------------
 * The reference has no incremental path: a moved MeshInstance3D means GeometryGroup3D::build() again
 * (geometry_group3d.cpp:78-366) and new ComputeShader buffers; its README lists a runtime TLAS update as wanted
 * (README.md:39-40).  Here the BLASes stay on the device; only the BLASInstance records
 * (BLASInstance::set_transform + update_aabb, bvh.h:81-115) and the TLAS (TLAS::build, bvh.cpp:264-317) are
 * redone and uploaded.  The result equals a fresh commit / upload of the moved scene. */
/*   route (ii): new Transform3D for instance `instance` (index in jpt_scene_add_instance order) ... */
int jpt_scene_set_instance_transform(jpt_ctx *ctx, uint32_t instance, const float *transform12);
/*   ... then one call that rebuilds instance records + TLAS with the builder of the last commit */
int jpt_scene_update_tlas(jpt_ctx *ctx);
/*   route (ii), on the device: ALL instance transforms at once (n_instances x 12 floats, jpt_scene_add_instance
 *   order).  Nothing is rebuilt on the host: one kernel recomputes the BLASInstance records from the transforms (the
 *   host builder's own arithmetic, bit for bit) and one refits the boxes of the TLAS records bottom-up over the
 *   topology of the last build.  They run on a stream of their own and write a COPY of the instance level that no
 *   render in flight reads (four copies: as many as renders in flight), so a queue of "refit, render" steps stays
 *   pipelined and the host never waits (jpt_scene_update_tlas drains the stream); the ctx stream is ordered after
 *   the refit.  Scenes committed with JPT_BUILD_SAH only; renders with the default kernel (the other kernels' arrays
 *   and jpt_scene_get_reference_buffer's host mirrors are refreshed by the next jpt_scene_update_tlas, which also
 *   re-optimises the topology: call it now and then when instances travel far).  The closest hit does not depend on
 *   the topology, so the image equals a fresh commit of the moved scene except at exact distance ties. */
int jpt_scene_refit_tlas(jpt_ctx *ctx, const float *transforms12, uint32_t n_instances);
/*   route (ii), on the device, with a NEW TOPOLOGY: jpt_scene_refit_tlas's arguments, state rules, error codes, fall-back and
 *   pipelining (the copy of the instance level no render reads, on the refit stream; the host waits for nothing but the one-time
 *   seeding of the copies and the reuse of a staging slot; renders queued before the call show the old scene, renders queued after
 *   it the new one) -- but the TLAS records are made anew: the instances are sorted on the device along a Morton curve through the
 *   centres of the world boxes their records just got (30 bits, the instance's index below them), and a fixed four-way tree over
 *   the sorted order -- a function of the instance count alone, so its root, refit schedule and stack need are known without asking
 *   the device -- takes them as its leaves.  Use it where a refit degrades: instances that swap places (debris, crowds, a shuffled
 *   grid) grow the boxes of the last commit's tree until every record near the root covers the scene.  The tree is a Morton tree,
 *   not jpt_scene_update_tlas's SAH tree (README: the measured difference); later refits, mesh updates and poses keep its topology,
 *   and jpt_scene_update_tlas afterwards rebuilds on the host from the kept transforms as ever.  At most 32 767 instances
 *   (JPT_E_LIMIT beyond; a tree deeper than the kernels' stack: JPT_E_LIMIT before anything is written); with one instance the call
 *   is the refit.  The first rebuild of an instance count uploads the tree's template (the host waits for it, once).  The image
 *   equals a fresh commit of the moved scene except at exact distance ties. */
int jpt_scene_rebuild_tlas(jpt_ctx *ctx, const float *transforms12, uint32_t n_instances);
/*   route (ii), on the device: new vertex positions (and normals) for mesh `mesh_id` (jpt_scene_add_mesh's id) of the
 *   committed scene; same surfaces, vertex counts and index arrays as at jpt_scene_add_mesh (otherwise: JPT_E_INVALID,
 *   "topology changed: commit the scene again").  Replaces GeometryGroup3D::build() of the whole scene, which is what a
 *   changed mesh costs in the reference (a skinned MeshInstance3D's surface arrays each frame).  Read: `vertices`, and
 *   `normals` when non-NULL (for every surface of the mesh or for none; NULL keeps the committed normals); `uvs` is not read,
 *   the committed uvs and material slots stay.  Kernels on the refit stream make the mesh's triangle records from the new
 *   vertices, refit the boxes of its BLAS records bottom-up over the topology of the last commit, and refit the instance level
 *   as jpt_scene_refit_tlas does with the current transforms; the vertices go through a pinned staging ring, so the host does
 *   not wait (except when a staging slot is reused).  The BLAS records are shared by every render, so the update waits on the
 *   device for every render queued before it: ONE PIPELINE DRAIN on the device per update; the renders queued after it wait
 *   for it.  The image of every later render equals a fresh JPT_BUILD_SAH_WATERTIGHT commit of the deformed scene except at
 *   exact distance ties; the topology stays the last commit's, so the boxes grow with the deformation -- jpt_scene_rebuild_mesh
 *   gives the mesh a new topology on the device, a new commit re-optimises the tree: call one now and then when a mesh deforms far.  JPT_BUILD_SAH_WATERTIGHT scenes only (JPT_E_STATE
 *   otherwise: JPT_BUILD_SAH's reach records and tie shadow are the reference builder's tree of the old vertices, and
 *   reference-exact trees are the reference's own).  Until the next jpt_scene_commit the host's copy of the scene is stale:
 *   jpt_scene_update_tlas, jpt_scene_share, jpt_scene_get_reference_buffer and renders with JPT_KERNEL_REFERENCE_LAYOUT or
 *   debug steps return JPT_E_STATE, and the sky cull is off; jpt_scene_refit_tlas keeps working.  A mesh that no instance
 *   names has nothing on the device: its update succeeds and changes nothing there.  Host-only contexts: JPT_E_DEVICE after
 *   the argument checks. */
int jpt_scene_update_mesh(jpt_ctx *ctx, uint32_t mesh_id, const jpt_surface *surfaces, int32_t n_surfaces);
/*   route (ii), on the device, with a NEW BLAS TOPOLOGY: jpt_scene_update_mesh's arguments, state rules, error codes and messages
 *   (with this call's name where a message names the call), its staging ring, its one pipeline drain on the device, the instance
 *   refit behind it and every restriction of a deformed scene (a JPT_BUILD_SAH_WATERTIGHT commit, the mesh's own topology of
 *   surfaces and indices, a stale host copy, the default kernel only, no sky cull) -- but the mesh's four-child records are made
 *   anew from the new vertices.  Use it where a refit degrades: cloth, a ragdoll, a morph between distant shapes, debris that lives
 *   in one mesh grow the leaf boxes of the last commit's tree until every record near the root covers the mesh.
 *
 *   The tree.  Triangle boxes: a triangle's box is the min and max of its three vertices taken one after the other from +-FLT_MAX
 *   ((b < a) ? b : a and (a < b) ? b : a, so a NaN coordinate is skipped).  Centres: per axis (lo + hi) * 0.5.  Bounds: per axis the
 *   min and max of the mesh's finite centres (an axis without one: +FLT_MAX .. -FLT_MAX).  Code: the 30-bit Morton code of
 *   jpt_scene_rebuild_tlas over the triangle's vertex box -- cell = min(1023, floor((centre - bmin) * inv)), inv = 1024 / (bmax -
 *   bmin) or 0 for an axis of no extent, a non-finite centre or product in cell 0, x in the highest bit of each triple; no float
 *   step of its own.  Order: ascending by (code, triangle index within the mesh) -- a stable sort by code; the order is unique, so
 *   any correct sort gives the same permutation.  Topology: jpt_debug_tlas_template's tree of n_tris sorted positions; a leaf slot
 *   over position p is the ONE triangle tri_first + sorted[p], its reference ~(int32_t)(tri_first + sorted[p]) (count 1).  The
 *   shading arrays are indexed by device triangle order: triangles are NOT reordered.  Boxes and quantised records: the refit's,
 *   bit for bit -- a leaf slot its triangle's vertex box widened by the mesh's padding, an internal slot the union of the record
 *   below, then jpt_debug_quantize_nodes4's form, then the mesh's root box.  A mesh of fewer than two triangles: the call is the
 *   refit.
 *
 *   Storage.  The tree has about n_tris / 3 records, more than the commit's SAH tree: the mesh's first rebuild reserves a region of
 *   that many records BEHIND the TLAS tails (every existing record keeps its index), points the root word of the mesh's instances
 *   at it, uploads the tree's template and sizes the sort's buffers; that first call may WAIT on the host for the renders queued
 *   before it.  After it no call waits for anything but the reuse of a staging slot.  The region is kept: later
 *   jpt_scene_update_mesh / jpt_scene_pose_mesh calls refit over the rebuilt topology, later rebuilds reuse it,
 *   jpt_debug_mesh_records reports it; the commit's range is no longer referenced.  jpt_scene_commit, an upload and jpt_scene_share
 *   INTO the context drop every region.  A tree deeper than the kernels' stack: JPT_E_LIMIT before anything is written or reserved.
 *
 *   The image of every later render equals a fresh JPT_BUILD_SAH_WATERTIGHT commit of the deformed scene except at exact distance
 *   ties.  The tree is a Morton tree with one-triangle leaves, not the commit's SAH tree (README, DESIGN.md section 5: the measured
 *   difference, which says when to refit, rebuild or commit).  Not covered: SAH or any treelet optimisation; leaves of more than one
 *   triangle; 63-bit codes; a host mirror of the rebuilt tree; JPT_BUILD_SAH and reference-exact scenes; returning the regions'
 *   memory before the next commit. */
int jpt_scene_rebuild_mesh(jpt_ctx *ctx, uint32_t mesh_id, const jpt_surface *surfaces, int32_t n_surfaces);
/*   route (ii), on the device, from a bone palette: what Godot computes for a MeshInstance3D with a Skeleton3D / Skin and an ArrayMesh's
 *   blend shapes (relative mode), done where the mesh refit reads its result.  jpt_scene_set_mesh_rig stores, once per mesh, what stays
 *   constant after the commit; jpt_scene_pose_mesh then takes the few numbers that change per frame and does jpt_scene_update_mesh's
 *   work with vertices a kernel computes on the device -- no per-vertex arithmetic, staging or copy on the host.
 *
 *   The arithmetic (gdpathtracing_amd/csrc/jpt_skin.h; binary32, one operation per + and *, in the order written, no fma).  Per vertex,
 *   from its bind position p and bind normal n: for every blend shape with a weight != 0, in ascending shape index, p = p + dP[s][v] * w
 *   per component and, when the rig has normal deltas, n = n + dN[s][v] * w.  Then, with `influences` = K > 0, the blended matrix M =
 *   B[b_0] * w_0 per entry, M = M + B[b_i] * w_i for i = 1 .. K-1 in order (every influence, zero weights included; the weights as
 *   given, not renormalised -- Godot does not either); x' = M[0]*x + M[1]*y + M[2]*z + M[9] left to right, y' from entries 3 4 5 10, z'
 *   from 6 7 8 11 (transform12 layout); the normal takes the same rows without the origin (the blended matrix, not its inverse
 *   transpose, as Godot).  With normals the output normal is normalised once at the end, as every normalize here: n * (1 / sqrt(n.n));
 *   a degenerate one is not checked.  B[b] = the bone's pose in skeleton space times the Skin's inverse bind matrix, multiplied by the
 *   caller: it maps a mesh-space bind position to a mesh-space posed position; instance transforms are not involved.
 *
 *   Not covered: dual-quaternion skinning, absolute (normalised-mode) blend shapes, tangents, per-instance poses (a mesh has ONE pose:
 *   its instances share the BLAS), and any SAH re-optimisation of the tree (jpt_scene_pose_mesh_rebuild gives it a new Morton topology; commit again for a SAH tree). */
typedef struct {
    const int32_t *bones;            /* n_vertices * influences   Mesh::ARRAY_BONES   (NULL when influences == 0) */
    const float   *weights;          /* n_vertices * influences   Mesh::ARRAY_WEIGHTS (NULL when influences == 0) */
    const float   *position_deltas;  /* n_blend_shapes * n_vertices * 3, shape-major  (NULL when n_blend_shapes == 0) */
    const float   *normal_deltas;    /* same shape, or NULL for every surface: normals are not morphed */
} jpt_surface_rig;
/*   The rig of mesh `mesh_id`: `bind` as jpt_scene_update_mesh's surfaces (same state rules, checks and messages: a
 *   JPT_BUILD_SAH_WATERTIGHT commit, the mesh's own topology) -- the bind-pose vertices, and normals for every surface or for none (none:
 *   the committed normals stay and normal deltas are refused); rigs[i] belongs to bind[i].  influences: 0 (no bones), 4 or 8
 *   (JPT_E_INVALID otherwise); n_blend_shapes <= 256 and bone indices in 0 .. 4095 (JPT_E_LIMIT); weights and deltas finite, and not
 *   influences == 0 with n_blend_shapes == 0 (JPT_E_INVALID).  The arrays are copied to the device once (bone indices packed to 16 bits,
 *   deltas shape-major over the whole mesh); the call waits for that copy and the caller's arrays are free on return.  A rig replaces
 *   the mesh's earlier one.  It is dropped by jpt_scene_begin, jpt_scene_commit, an upload, jpt_scene_share INTO the context and
 *   jpt_destroy; jpt_scene_share does not carry rigs to dst.  A mesh that no instance names is accepted and stores nothing on the
 *   device.  Host-only contexts: JPT_E_DEVICE after the argument checks. */
int jpt_scene_set_mesh_rig(jpt_ctx *ctx, uint32_t mesh_id, const jpt_surface *bind, const jpt_surface_rig *rigs,
                           int32_t n_surfaces, int32_t influences, int32_t n_blend_shapes);
/*   One pose of a rigged mesh: n_bones transform12 records (48 B per bone; NULL / 0 for a rig without bones) and one weight per blend
 *   shape of the rig.  JPT_E_STATE unless the scene is a JPT_BUILD_SAH_WATERTIGHT commit (jpt_scene_update_mesh's state rules, checked
 *   here too) and without a rig; JPT_E_INVALID unless n_bones exceeds the rig's largest bone index (this check keeps
 *   the kernel's gather inside the palette), n_blend_weights equals the rig's shape count and the weights are finite.  The palette is
 *   not inspected, as jpt_scene_update_mesh does not inspect vertices.  The bounds head, the palette and the shapes with a weight != 0
 *   go through the pinned ring of jpt_scene_update_mesh; one kernel (one thread per vertex) writes the posed vertices and normals,
 *   beside the renders still in flight; from there on the call IS jpt_scene_update_mesh: one pipeline drain on the device, the mesh's
 *   records and the instance level refitted, and every restriction of a deformed scene documented there (a stale host copy, the
 *   default kernel only, no sky cull).  A render queued before the call shows the previous pose, one queued after it the new one.
 *   A pose of a mesh that no instance names changes nothing, on the device or in the context: the host's copy of the scene stays
 *   current. */
int jpt_scene_pose_mesh(jpt_ctx *ctx, uint32_t mesh_id, const float *bone_transforms12, uint32_t n_bones,
                        const float *blend_weights, uint32_t n_blend_weights);
/*   jpt_scene_pose_mesh with a NEW BLAS TOPOLOGY: its arguments, checks and messages (under this call's name), and behind the skin
 *   kernel the call IS jpt_scene_rebuild_mesh over the posed vertices -- the tree, the region and the first call's wait as there. */
int jpt_scene_pose_mesh_rebuild(jpt_ctx *ctx, uint32_t mesh_id, const float *bone_transforms12, uint32_t n_bones,
                                const float *blend_weights, uint32_t n_blend_weights);
/*   Drops the rig of `mesh_id` (no rig: nothing happens); the mesh keeps its last pose. */
int jpt_scene_clear_mesh_rig(jpt_ctx *ctx, uint32_t mesh_id);
/*   route (i): the caller re-ran BLASInstance::set_transform / TLAS::build itself; same instance count and
 *   the same blas_index per instance as the uploaded scene (otherwise: JPT_E_INVALID, upload the whole scene) */
int jpt_scene_update_reference_tlas(jpt_ctx *ctx, const void *blas_instances, uint32_t n_instances,
                                    const void *tlas_nodes, uint32_t n_tlas_nodes);

/* ---- per-render state ------------------------------------------------------------------------- */

/* replaces: Params upload (RenderParameters, path_tracing_camera.cpp:129-133,142; only width/height are
 * read by the shader, main.glsl:407,411), the literal 5 of main.glsl:377 (= max_bounces + 1), and the
 * rgba8 / r32f / rgba32f image creation (path_tracing_camera.cpp:148-165, progressive_rendering.cpp:35-39). */
int jpt_set_params(jpt_ctx *ctx, int32_t width, int32_t height, int32_t max_bounces,
                   int32_t accum_mode, int32_t sampler_mode);

/* Lighting from an HDR environment map instead of main.glsl's fixed sky gradient (no reference counterpart; the reference
 * lists a sky HDRI among its wanted features).  Without a map -- the default, and after jpt_set_environment(ctx, NULL, 0, 0)
 * -- every render is exactly what it was: the same kernels, the same bits.
 *   rgb: `height` rows of `width` texels, 3 linear floats each, finite and >= 0, row 0 the +y pole, columns the longitude
 *        (equirectangular, the layout of a Radiance .hdr panorama; gdpathtracing_amd.hdrio / jpt_host.hpp load_hdr read one).
 *        At most 16384 x 8192 texels (JPT_E_LIMIT beyond); bad sizes, NaN, infinities or negative texels: JPT_E_INVALID.
 *        The map belongs to the context, like jpt_set_params: it survives scene commits, uploads, jpt_scene_update_tlas,
 *        jpt_scene_refit_tlas and jpt_scene_update_mesh; jpt_scene_share does not copy it.  The call WAITS for the renders the
 *        context has queued (they finish with the old map) before it frees the old map and copies the new one (16 B per texel
 *        on the device).  Host-only contexts: JPT_E_DEVICE after the checks.
 * A ray that leaves the scene adds throughput * env_radiance(d), d its world direction: m = R d, phi = atan2(m.x, -m.z),
 * theta = atan2(|m.xz|, m.y), bilinear between the texel centres at ((phi / 2pi + 1/2) width - 1/2, theta / pi height - 1/2),
 * columns wrapping, rows clamped, times the intensity -- a fixed sequence of binary32 operations, the same
 * on every kernel, tree kind, upload route and denoising mode.  In JPT_ACCUM_REF_LDR8 mode each frame is clamped to 8 bits as
 * always, so a bright sun in the map is clamped per frame to 1.0; use JPT_ACCUM_HDR_F32 to keep its energy.  The map is
 * reached by BRDF sampling alone unless jpt_set_environment_sampling(ctx, JPT_ENV_SAMPLING_MIS) adds importance sampling of
 * the map with shadow rays (below): without it small bright suns converge slowly.  The debug-steps image has no sky and ignores the map. */
int jpt_set_environment(jpt_ctx *ctx, const float *rgb, int32_t width, int32_t height);
/* rotation9: row-major 3x3 world -> map (NULL: identity; each row's dot product is summed left to right), intensity: finite
 * and >= 0 (default 1).  Passed by value with every later render: changing them (a time-of-day rotation every frame) never
 * waits for queued renders.  Non-finite entries or a negative intensity: JPT_E_INVALID; host-only contexts: JPT_E_DEVICE
 * after the checks. */
int jpt_set_environment_params(jpt_ctx *ctx, const float *rotation9, float intensity);

/* Importance sampling of the environment map (no reference counterpart; the reference lists next-event estimation among its
 * wanted features).  The mode belongs to the context, like the map: it survives scene commits, uploads, jpt_scene_update_tlas,
 * jpt_scene_refit_tlas and jpt_scene_update_mesh; jpt_scene_share does not copy it.  Each render takes it by value: queued
 * renders keep the mode of their own call.
 *   JPT_ENV_SAMPLING_BRDF (default)  the map is reached by BRDF sampling alone: the same kernels and bits as without this call.
 *   JPT_ENV_SAMPLING_MIS             every hit below the last bounce (bounce < max_bounces) also draws one direction l from the
 *        map's own distribution and casts a shadow ray from position + normal * 0.001 (no t limit); unoccluded and with n.l > 0
 *        it adds throughput * brdf(l) * n.l * L_env(l) * w_env / p_env(l); a BRDF-sampled miss at bounce >= 1 adds its
 *        radiance times w_brdf = p_brdf^2 / (p_brdf^2 + p_env^2) (the power heuristic; a primary miss keeps weight 1).  Where
 *        p_env = 0 the BRDF sample covers the direction alone: the estimator stays unbiased and small bright suns converge in
 *        a few frames.  The distribution is piecewise constant over the texels, each weighing its luminance (0.2126 r +
 *        0.7152 g + 0.0722 b) times sin theta at its row's centre; p_env(d) = (weight / total) * width * height /
 *        (2 pi^2 sin theta), the texel being the one the lookup's mapping puts d in.  The NEE randoms
 *        come from a hashed copy of the vertex's seeds, so every BRDF-sampled continuation is the one BRDF mode takes.
 *        "Blocked" means the pipeline's closest-hit query along the shadow ray finds a triangle (t <= 1e9): on the native
 *        trees the brute-force answer, on the reference-layout tree (JPT_KERNEL_REFERENCE_LAYOUT) that tree's answer, without
 *        reach or tie logic in either.  The sampler needs an orthonormal rotation: with MIS on, jpt_set_environment_params
 *        refuses one whose R R^T is further than 1e-4 from the identity in any entry (JPT_E_INVALID), and so does this call
 *        when it enables MIS.  Without a map, or with an all-black one, MIS renders are BRDF renders.
 * The tables (4 B per texel + 4 B per row on the device) are built on the device when they are first needed -- at this call
 * with a map present, or at jpt_set_environment while MIS is on -- and this is the one case in which the call waits for the
 * context's queued renders; they are kept until the map changes, so switching back and forth never waits.  An MIS render's
 * workspace holds a shadow-ray queue (48 B per queue entry) and 4 B per path more (jpt_get_workspace_bytes counts them
 * while MIS is on).  A bad mode: JPT_E_INVALID; host-only contexts: JPT_E_DEVICE after the checks. */
#define JPT_ENV_SAMPLING_BRDF 0
#define JPT_ENV_SAMPLING_MIS  1
int jpt_set_environment_sampling(jpt_ctx *ctx, int32_t mode);

/* A procedural sky made on the device (no reference counterpart): the environment map of a gradient sky -- the form of Godot 4's
 * ProceduralSkyMaterial without its cover texture -- written into the context's map buffer by a kernel, from about 200 bytes of
 * parameters.  After the call the context holds an environment map like any other: the lookup, jpt_set_environment_params,
 * jpt_set_environment_sampling, every camera, bake and probe form, jpt_scene_share not copying it and
 * jpt_set_environment(ctx, NULL, 0, 0) clearing it behave as for an uploaded map; jpt_set_environment(rgb) replaces it.
 *   Texel (i, j) is the mean of samples x samples values of sky_radiance at the directions the lookup maps to an even grid inside
 *   the texel (csrc/jpt_sky.h).  For a unit direction d at polar angle theta from +y, b = theta / (pi / 2):
 *     d.y >= 0: c = mix(sky_horizon, sky_top, w(b, sky_curve)) * sky_energy; then for each sun in order, a the angle between d and
 *               the sun: a < radius: c = the disk's radiance; else a < amax = max(sun_angle_max, radius):
 *               c = mix(disk, c, w(1 - (a - radius) / (amax - radius), sun_curve));
 *     d.y <  0: c = mix(ground_horizon, ground_bottom, w(2 - b, ground_curve)) * ground_energy (suns do not show below the horizon);
 *     w(b, curve) = clamp(1 - pow(clamp(b, 0, 1), 1 / curve), 0, 1); the result is c * exposure.
 *   A fixed sequence of binary32 operations, the same on the device and in the host forms below.
 * Checks (JPT_E_INVALID, the message names the field): colours, energies and exposure finite and >= 0; curves in [1/64, 8];
 * sun_angle_max in [0, pi]; n_suns in 0..4; a sun's direction finite and non-zero, its radius in (0, pi/2], its mode known; samples
 * in 1..8; sizes positive.  Beyond 16384 x 8192 texels: JPT_E_LIMIT.  Host-only contexts: JPT_E_DEVICE after the checks.
 * When the context already holds a map of this size (made by either call) the kernel is queued on the context's stream, behind the
 * renders already queued, and the next render of every pipeline slot is ordered after it: the host does NOT wait, a render queued
 * before the call shows the old sky, one queued after it the new one -- a time-of-day animation costs a kernel per change.
 * Otherwise the call waits for the queued renders and allocates, as jpt_set_environment does.  With JPT_ENV_SAMPLING_MIS on, the
 * sampling tables are rebuilt at this call and the call waits for their total, as jpt_set_environment does.
 * Through JPT_ENV_SAMPLING_MIS a sun disk in the map is a directional light with soft shadows; its sharpness is limited by the
 * texel size (a 0.27 degree sun wants 4096 x 2048 or more).  Use JPT_ACCUM_HDR_F32 to keep a sun's energy. */
enum { JPT_SUN_RADIANCE = 0, JPT_SUN_IRRADIANCE = 1 };
typedef struct jpt_sky_sun {
    float direction[3];     /* from the scene towards the sun, map frame (world when the rotation is identity); any length > 0 */
    float angular_radius;   /* radians, (0, pi/2] */
    float color[3];         /* linear, finite, >= 0 */
    float energy;           /* finite, >= 0 */
    int32_t mode;           /* RADIANCE: the disk's radiance is color*energy (Godot's look).  IRRADIANCE: color*energy /
                               (2 pi (1 - cos r)), computed in double: the disk alone sends color*energy of irradiance onto a
                               surface that faces it -- the stand-in for a DirectionalLight3D */
} jpt_sky_sun;
typedef struct jpt_sky_params {
    float sky_top_color[3], sky_curve, sky_horizon_color[3], sky_energy;
    float ground_bottom_color[3], ground_curve, ground_horizon_color[3], ground_energy;
    float sun_angle_max, sun_curve, exposure;
    int32_t n_suns;         /* 0..4 */
    jpt_sky_sun suns[4];
} jpt_sky_params;
/* Godot 4's defaults: sky top (0.385, 0.454, 0.55), both horizons (0.6463, 0.6558, 0.6708), ground bottom (0.2, 0.169, 0.133), sky
 * and sun curve 0.15, ground curve 0.02, energies and exposure 1, sun_angle_max 30 degrees, no sun */
void jpt_sky_defaults(jpt_sky_params *out);
int jpt_set_sky(jpt_ctx *ctx, const jpt_sky_params *params /* NULL: the defaults */, int32_t width, int32_t height, int32_t samples);
/* The map the context holds, made by jpt_set_environment or jpt_set_sky: three floats per texel in jpt_set_environment's layout.
 * rgb may be NULL (sizes only).  Waits for the context's stream.  Without a map: JPT_E_STATE. */
int jpt_read_environment_f32(jpt_ctx *ctx, float *rgb /* may be NULL: sizes only */, int32_t *width, int32_t *height);

/* Importance sampling of the emissive triangles (no reference counterpart; the reference lists next-event estimation among its
 * wanted features).  The mode belongs to the context, like the map's: it survives scene commits, uploads and updates;
 * jpt_scene_share does not copy it.  Each render takes it by value: queued renders keep the mode of their own call.
 *   JPT_LIGHT_SAMPLING_BRDF (default)  emitters are reached by BRDF sampling alone: the same kernels and bits as without this call.
 *   JPT_LIGHT_SAMPLING_MIS             the emitters are sampled directly and combined with BRDF sampling by the power heuristic.
 * Emitters: every (instance, triangle) pair whose Le -- emission.rgb * max(0, emission.w) of the material get_shading_data looks
 *   up for it (an out-of-range index: material 0) -- has lum(Le) = 0.2126 r + 0.7152 g + 0.0722 b > 0, listed instance by
 *   instance, each instance's triangles (those under its BLAS root) in ascending index.  Power = lum(Le) * world area, the area
 *   0.5 |E1 x E2| of the world edges E1 = xform_dir(transform, v1 - v0), E2 likewise, vertex 0 P0 = xform_point(transform, v0);
 *   a power that is not finite and > 0 (zero-area, degenerate) is 0 and never drawn.  Tables: blocks of 256 emitters, per block
 *   a sequential prefix sum of the powers normalised by the block's total (the last entry exactly 1; a block of power 0: all 1s),
 *   and the same over the block totals in block order; their sum is the total.  When the scene's total is 0 (no emitter) MIS
 *   renders are BRDF renders.
 * Estimator, at every hit with bounce < max_bounces (total > 0): randoms from a copy of the vertex's seeds hashed by two pcg2d
 *   rounds of (sx ^ 0x2c1b3c6d, sy ^ 0x297a2d39) -- the path's own sequence, so its BRDF continuation, is that of BRDF mode;
 *   xi0 (clamped below 1) picks the block on the marginal CDF and xi1 (clamped) the emitter on the block's CDF (the first entry
 *   > xi); s = sqrt(xi2), y = (P0 + E1 * (s * (1 - xi3))) + E2 * (s * xi3).  o = position + normal * 0.001, l = normalize(y - o),
 *   d2 = dot(y - o, y - o), c = |normalize(E1 x E2) . l| (emission is two-sided);
 *   p_L = (lum(Le) * d2) / (total * c), w_L = p_L^2 / (p_L^2 + p_brdf(l)^2).  When n.l > 0, c > 0 and the contribution
 *   ((throughput * (brdf(l) * n.l)) * Le) * (w_L / p_L) is finite with a component > 0, a shadow ray (o, l) with
 *   tmax = sqrt(d2) * 0.9999f is cast; it is blocked when some triangle's Moller-Trumbore test accepts t < tmax (the closest-hit
 *   walk started with t = tmax ends below it): on the native trees the brute-force answer, on the reference-layout tree
 *   (JPT_KERNEL_REFERENCE_LAYOUT) that tree's answer, without reach or tie logic.  Unblocked, the contribution is added.
 *   Emission that a BRDF-sampled ray (origin o, direction d) finds at bounce >= 1 is weighted by p_brdf^2 / (p_brdf^2 + p_L^2),
 *   p_brdf the previous vertex's density of d, p_L as above with d2 = |position - o|^2 and the hit triangle's world edges (a NaN
 *   weight is 1); non-emitters and primary hits keep weight 1.  With JPT_ENV_SAMPLING_MIS as well, a vertex casts the map's
 *   shadow ray and then the emitters' and their contributions join the path in that order; each estimator is weighted against
 *   BRDF sampling alone.
 * The emitter list follows the scene the renders see: it is made from the committed or uploaded scene (and again after
 * jpt_scene_update_tlas / jpt_scene_update_reference_tlas); the tables are rebuilt on the device at the first render that samples
 * them after any change, jpt_scene_refit_tlas and jpt_scene_update_mesh included, ordered after the renders already queued.  In
 * BRDF mode none of this runs.  Memory: 8 B per emitter for the list (on the host and on the device), 52 B per emitter and 4 B
 * per 256 for the tables; a
 * light-sampling render's workspace holds a second shadow-ray queue (48 B per queue entry) and, without map MIS, 4 B per path
 * (jpt_get_workspace_bytes counts them).  A bad mode: JPT_E_INVALID; host-only contexts: JPT_E_DEVICE after the checks. */
#define JPT_LIGHT_SAMPLING_BRDF 0
#define JPT_LIGHT_SAMPLING_MIS  1
int jpt_set_light_sampling(jpt_ctx *ctx, int32_t mode);

/* Material extensions: transparent materials (no reference counterpart; the reference lists them among its wanted features).
 * GpuMaterial ends in float padding[5], which a stock addon leaves uninitialised: by default those bytes are never read.  With
 * JPT_MATERIAL_EXT_TRANSMISSION set, padding[0] is `transmission` and padding[1] is `ior` of every material (jpt_material_ext), on
 * both ingest routes; the device sanitises them: transmission NaN -> 0, then clamped to [0, 1]; ior NaN -> 1, then clamped to [1, 4].
 * The flags belong to the context, like the sampling modes: they survive scene commits, uploads and updates; jpt_scene_share does
 * not copy them.  Each render takes them by value: queued renders keep the flags of their own call.  With the flag off, or on over
 * a scene none of whose materials has a sanitised transmission > 0, a render launches the kernels and gives the bits it gives
 * without this call; otherwise it launches the general *_tx kernels, whatever the lighting.
 * The vertex, at a hit whose material has T = transmission > 0, after emission is added as always: one pcg2d round of a copy of
 *   the vertex's seeds hashed as (sx ^ 0x5bd1e995, sy ^ 0x1b873593) gives (xi_t, xi_f); the path's own sequence does not advance
 *   for this.  xi_t >= T: the vertex is the opaque vertex, unchanged (probability 1 - T and weight 1 - T cancel).  Otherwise a
 *   smooth dielectric event (dielectric_event, csrc/jpt_shade.h; DESIGN.md section 2 pins every operation): n the facing shading
 *   normal, v the direction back along the ray, m = n (or -n when n.v < 0), c = min(|n.v|, 1), eta = 1 / ior at a front face, ior
 *   at a back face, k = 1 - eta^2 (1 - c^2).  k < 0: total internal reflection.  Otherwise ct = sqrt(k) and F the exact
 *   unpolarised Fresnel reflectance (not finite or > 1: 1).  TIR or xi_f < F: d = 2 c m - v from position + n * 0.001, throughput
 *   unchanged.  Otherwise d = normalize((eta c - ct) m - eta v) from position - n * 0.001, throughput *= albedo (the material's
 *   albedo times its texture: the tint).  Radiance is NOT scaled by eta^2 across the interface.  The path never ends at such a
 *   vertex; its own pcg2d draw is taken and discarded.  A dielectric vertex casts no shadow ray, and the emission or the miss the
 *   next vertex finds has MIS weight exactly 1.  Shadow rays stay opaque to glass: light through glass arrives by BSDF sampling.
 * Unknown bits: JPT_E_INVALID; host-only contexts: JPT_E_DEVICE after the checks.  Memory: a *_tx render's workspace holds 4 B
 * per path more than the same lighting's without it, unless that already holds them (jpt_get_workspace_bytes counts them). */
enum { JPT_MATERIAL_EXT_NONE = 0, JPT_MATERIAL_EXT_TRANSMISSION = 1 };
typedef struct jpt_material_ext {   /* documentation of GpuMaterial's first two padding words under JPT_MATERIAL_EXT_TRANSMISSION */
    float transmission;             /* padding[0]: the probability of the dielectric lobe, [0, 1] */
    float ior;                      /* padding[1]: the index of refraction of the inside, [1, 4] */
} jpt_material_ext;
int jpt_set_material_extensions(jpt_ctx *ctx, uint32_t flags);

/* The thin-lens camera: depth of field (no reference counterpart; Godot's CameraAttributesPhysical / Practical carry a focus
 * distance and an aperture -- INTEGRATION.md maps them onto this call).  aperture_radius: the radius of the lens disk in world
 * units, finite and >= 0; 0 (the default) is the pinhole.  focus_distance: the distance from cam.position, along the camera's
 * forward axis, of the plane that stays sharp, finite and > 0; not read when the radius is 0.  Anything else: JPT_E_INVALID;
 * host-only contexts: JPT_E_DEVICE after the checks.
 * The lens belongs to the context, like the sampling modes: it survives scene commits, uploads and updates, jpt_set_camera and
 * jpt_set_params; jpt_scene_share does not copy it.  Each render takes it by value: queued renders keep the lens of their own
 * call, and setting it never waits.  With radius 0 a render launches the kernels it launches without this call and gives the same
 * bits.  With a lens the bounce-0 launch is the lens form of its kernel (wf2_primary_lens / wf2_primary_env_lens; the audit kernel
 * branches) and the render has no sky cull (jpt_stats.sky_culled is 0): a pixel whose pinhole ray misses every box may still see
 * geometry from a point of the aperture.  Every later launch, the workspace and jpt_get_workspace_bytes are the pinhole's.
 * The camera basis is derived from camera160 at each render (a host that moves the camera calls nothing extra): with unproject(nx,
 *   ny) = ivp * (nx, ny, 1, 1) / w as the primary ray forms it, c0 = unproject(0, 0), f = normalize(c0 - position), c1 =
 *   unproject(1, 0), r0 = c1 - c0, r = normalize(r0 - f (r0 . f)), u = r x f -- for a Godot camera forward -z, right +x, up +y.
 *   A basis with a non-finite component: the render calls return JPT_E_STATE with a message.
 * The path, after the pinhole ray (o, d) of its pixel and frame is made and the jitter draw has left the seeds (sx, sy): one pcg2d
 *   round of a copy of the seeds hashed as (sx ^ 0x85ebca6b, sy ^ 0xc2b2ae35) gives (xi0, xi1); the path's own sequence does not
 *   advance, so every later vertex draws what it draws under the pinhole.  rad = radius sqrt(xi0), (lu, lv) = rad (cos, sin)(2 pi
 *   xi1); cf = d . f; !(cf > 0): the pinhole ray is kept.  Otherwise p = o + d (focus / cf), o' = (o + r lu) + u lv, d' =
 *   normalize(p - o') (csrc/jpt_lens.h; DESIGN.md section 2 pins every operation).
 * JPT_DENOISE_TEMPORAL with a lens: the render calls return JPT_E_STATE (the reprojection assumes one centre of projection).
 * jpt_set_debug_steps ignores the lens, as it ignores lighting.  jpt_denoise runs on a lens render; its guide pass stays the
 * un-jittered pinhole ray through the pixel centre (guides of the sharp scene: a blurred edge is filtered as the edge it is in
 * focus).  The depth image holds the distance from the ray's origin on the lens, not from cam.position. */
int jpt_set_lens(jpt_ctx *ctx, float aperture_radius, float focus_distance);

/* The camera model: how a raster position becomes a primary ray (no reference counterpart: the reference, too, shoots every ray
 * from cam.position, which is a wrong picture under an orthographic matrix).
 *   PINHOLE      (default) from cam.position towards ivp * (nx, ny, 1, 1): right for a perspective Projection.  The launches, the
 *                kernels and the bits of a context that never made this call.
 *   PROJECTIVE   from the position's point on the near plane, ivp * (nx, ny, -1, 1), towards its point on the far plane, ivp * (nx,
 *                ny, +1, 1) (each divided by its own w; the GL-style z range of Godot's Projection).  Exact for Godot's
 *                PROJECTION_ORTHOGONAL (parallel rays); for a perspective matrix the pinhole's directions with near-plane clipping;
 *                right for PROJECTION_FRUSTUM and any other invertible projection.
 *   EQUIRECT     the full sphere around cam.position, in the layout jpt_set_environment reads: with u = x / width, v = y / height,
 *                phi = (u - 1/2) 2 pi, theta = v pi, the direction r sin(theta) sin(phi) + u cos(theta) + f sin(theta) cos(phi) over the
 *                camera basis (f, r, u) jpt_set_lens derives from camera160 -- row 0 is the camera's up pole, the centre column
 *                forward, columns increase to the right.  With the identity camera this is the map's (sin theta sin phi, cos theta,
 *                -sin theta cos phi): a panorama rendered at a point is, as it is, an environment map for that point.
 * The seed and the jitter of a path are the pinhole's, draw for draw, so every later vertex draws what it draws under the pinhole
 * (csrc/jpt_camera.h; DESIGN.md section 2 pins every operation).  A value that is none of the three: JPT_E_INVALID; host-only
 * contexts: JPT_E_DEVICE after the check.
 * The model belongs to the context, like the lens: it survives scene commits, uploads, refits and mesh updates, jpt_set_camera and
 * jpt_set_params; jpt_scene_share does not copy it.  Each render takes it by value: queued renders keep the model of their own call.
 * A render under PROJECTIVE or EQUIRECT launches the model's form of its bounce-0 kernel (wf2_primary_cam / wf2_primary_env_cam; the
 * audit kernel branches) and has no sky cull (jpt_stats.sky_culled is 0); every later launch, the workspace and
 * jpt_get_workspace_bytes are the pinhole's.  The depth image holds the distance from the ray's own origin.
 * The render calls return JPT_E_STATE, with a message, for a model other than PINHOLE with a lens radius > 0 (the disk is defined
 * around one centre of projection) or under JPT_DENOISE_TEMPORAL, for EQUIRECT with a basis that is not finite and for PROJECTIVE
 * with an ivp that is not finite.  jpt_set_debug_steps ignores the model, as it ignores the lens.
 * jpt_denoise builds its guides from the model's ray through the pixel centre, and jpt_query_pixels forms the model's ray of each
 * raster position (the same two JPT_E_STATE cases apply to both); jpt_query_rays and jpt_query_rays_device take rays as given. */
enum { JPT_CAMERA_PINHOLE = 0, JPT_CAMERA_PROJECTIVE = 1, JPT_CAMERA_EQUIRECT = 2 };
int jpt_set_camera_model(jpt_ctx *ctx, int32_t model);

/* Lightmap baking: paths from surface texels instead of camera pixels (no reference counterpart; Godot's LightmapGI wants a lightmap
 * per mesh over its UV2 channel).  Two device images of width * height * 4 floats each say where the texels are -- 32 B per texel of
 * device memory, not counted by jpt_get_workspace_bytes:
 *   position4 = (world position, w)      normal4 = (world normal, w)       (w is not read; the rasteriser writes the triangle, and 1)
 * A texel is VALID when dot(n.xyz, n.xyz) > 0 (NaN fails the test); all zeros is the canonical invalid texel.  While a context holds
 * images its renders are BAKE RENDERS: the path of texel (x, y) starts at position + nh * 0.001, nh the normalised normal, leaves in
 * a cosine-distributed direction about nh and carries throughput 1, so accum.rgb / frame_count in JPT_ACCUM_HDR_F32 mode converges
 * to E / pi, E the irradiance at the texel: the radiance a white Lambertian surface sends back, which is what a lightmap stores
 * (multiply by the albedo in the engine).  An invalid texel traces nothing: radiance 0, first-hit distance far, no ray counted.
 * The seed and the jitter draw of a path are the camera's, draw for draw; the direction's two randoms come from one pcg2d round of a
 * copy of the seeds hashed as (sx ^ 0x3c6ef372, sy ^ 0xa54ff53a), so every later vertex draws what it draws under a camera
 * (csrc/jpt_bake.h; DESIGN.md section 2 pins every operation).  Nothing downstream of the first ray knows: the shading, occlusion and
 * accumulation kernels, environment maps, both MIS modes, glass, the 8-row partition, jpt_multi, every read-back, jpt_display and
 * jpt_meter work on a bake render as on a picture.  The depth image holds the usual reversed-Z value of the distance from the ray's
 * origin.  A bake render launches the bake form of its bounce-0 kernel (wf2_primary_bake / wf2_primary_env_bake; the audit kernel
 * branches), has no sky cull (jpt_stats.sky_culled is 0), and every later launch and the workspace are the camera's.
 *
 * jpt_set_bake_texels    uploads both images; (NULL, NULL, 0, 0) frees them: renders are camera renders again, with the launches and
 *                        the bits of a context that never baked.  A valid texel with a non-finite position or normal component:
 *                        JPT_E_INVALID.
 * jpt_bake_begin         allocates width x height images, every texel invalid, for jpt_bake_add_surface to fill.
 * jpt_bake_add_surface   rasterises one surface's UV2 triangles (uv2: n_vertices * 2 floats, Mesh::ARRAY_TEX_UV2, the image is [0, 1]^2,
 *                        row 0 at v = 0) through transform12 (the instance's, as jpt_scene_add_instance reads it) into the images, on
 *                        the device: a texel whose CENTRE (x + 1/2, y + 1/2) lies inside or on the edge of a triangle with a UV2 area
 *                        other than 0 gets the position and the normalised normal interpolated there (position4.w = the triangle's
 *                        number, normal4.w = 1), or becomes invalid when a component is not finite.  Within a call the lowest
 *                        triangle number wins a texel; a later call replaces what its own triangles cover and leaves the rest; the
 *                        result does not depend on the order the device's threads run in.  surface->uvs is not read.  n_indices no
 *                        multiple of 3, an index out of range or a null array: JPT_E_INVALID; more than 2^24 triangles: JPT_E_LIMIT.
 * jpt_read_bake_texels   copies the images out; either pointer may be NULL.
 * All sizes must be >= 1 (JPT_E_INVALID) and width * height at most 2^26 texels (JPT_E_LIMIT).  jpt_bake_add_surface and
 * jpt_read_bake_texels without images: JPT_E_STATE.  Host-only contexts: JPT_E_DEVICE after the checks.
 * The three writing calls WAIT for the renders the context has queued, which finish with the old images, and return when the images
 * are written: queued renders keep the images of their own call.  The images belong to the context, like the environment map: they
 * survive scene commits, uploads, refits and mesh updates; jpt_scene_share does not copy them.
 * The render calls return JPT_E_STATE, with a message, while images are present and their size is not jpt_set_params' width x height
 * (every rank of a partition holds the whole images), the lens radius is > 0, the camera model is not JPT_CAMERA_PINHOLE or the
 * denoising mode is JPT_DENOISE_TEMPORAL.  jpt_set_debug_steps ignores the images, as it ignores the lens.  jpt_denoise and
 * jpt_query_pixels return JPT_E_STATE while images are present: their guide and picking rays are camera rays.
 * jpt_bake_finish (below) filters and dilates the accumulated map on the device.
 * Out of scope: conservative coverage (a triangle that covers no texel centre leaves no texel), seam stitching across UV islands,
 * atlas packing, next-event estimation at the texel itself (direct light reaches a texel by its first ray alone, so small emitters
 * converge slowly).  (Directional lightmaps: jpt_set_bake_directional, below.  Light probes: jpt_set_probes, below.) */
int jpt_set_bake_texels(jpt_ctx *ctx, const float *position4, const float *normal4, int32_t width, int32_t height);
int jpt_bake_begin(jpt_ctx *ctx, int32_t width, int32_t height);
int jpt_bake_add_surface(jpt_ctx *ctx, const jpt_surface *surface, const float *uv2, const float *transform12);
int jpt_read_bake_texels(jpt_ctx *ctx, float *position4, float *normal4);

/* ---- finishing a baked lightmap: chart-aware filter and dilation (no reference counterpart; Godot's LightmapGI denoises and dilates
 * after tracing) ----
 * The accumulation of a bake render is noisy, and zero outside every chart, so bilinear sampling pulls black in across every UV seam.
 * jpt_bake_finish makes the map an engine can sample, as an explicit call like jpt_denoise: nothing runs unless the host asks, and
 * without the call every render, buffer and read-back is bit for bit what it is today.  No guide pass is traced: the bake images are
 * the world position and normal of every texel.  The arithmetic is pinned ("finishing a lightmap";
 * gdpathtracing_amd/csrc/jpt_lightmap.h; tests/np_lightmap.py restates it bit for bit):
 *   prepare   per texel: valid as a bake render decides; guides (position, fp2) and (normalised normal, 0), fp2 the texel's squared
 *             world footprint = the LEAST squared distance to a valid 4-neighbour (0: none); colour i_0 = (accum.rgb / frame_count, 1),
 *             or (0, 0, 0, 0) for an invalid texel.  No albedo demodulation: a bake path carries throughput 1.
 *   filter    `passes` a-trous passes over the valid texels, 5 x 5 binomial taps at spacing 2^k.  A tap counts only when it is valid and
 *             its world distance is at most sigma_distance times its atlas distance measured in footprints (d2 <= sigma_distance^2 *
 *             r2, r2 = (2^k)^2 (dx^2 + dy^2) fp2) -- two charts that touch in the atlas do not mix -- and then weighs
 *             max(0, n_p . n_q)^(2^normal_power_log2) * max(0, 1 - (n_p . d)^2 / (sigma_plane^2 r2)) * 1 / (1 + |dc|^2 / sc^2),
 *             sc = sigma_color halved every pass.  Non-finite colours are skipped as taps and pass through as centres.
 *   dilate    `dilate` passes, each reading only the one before: a texel of coverage 0 with a neighbour of coverage > 0 among its 8
 *             takes their mean (weight 2 for the four edge neighbours, 1 for the diagonals) and coverage 0.5.
 *   output    (r, g, b, coverage): coverage 1 for a valid texel, 0.5 for a dilated one, 0 (and colour 0) for an untouched one.
 *
 * jpt_bake_finish enqueues on the context's stream exactly as jpt_denoise does: behind every render queued before it and ahead of
 * those queued after it.  It READS the accumulation, the frame count and the bake images and writes only its own images: 64 B per
 * texel (two guide images, a colour ping and pong), allocated at the first call at a size, freed by jpt_set_params with another size,
 * by every call that writes the bake images (jpt_set_bake_texels, jpt_bake_begin, jpt_bake_add_surface) and by jpt_destroy; not
 * counted by jpt_get_workspace_bytes.
 * JPT_E_STATE, with a message naming the call: no bake images; their size is not jpt_set_params'; no frame accumulated since the last
 * reset; a denoising mode other than JPT_DENOISE_PROGRESSIVE; DEBUG_STEPS mode; a screen partition.  jpt_read_lightmap_f32 before a
 * jpt_bake_finish at the current size and images: JPT_E_STATE.  A parameter outside its range or not finite: JPT_E_INVALID.  Host-only
 * contexts: JPT_E_DEVICE after the checks that need no device.  There is no jpt_multi_* form, as for jpt_denoise.
 * The parameters are the context's (like jpt_set_denoise_params'): they survive scene changes, each jpt_bake_finish takes them by
 * value, jpt_scene_share does not copy them.
 * Out of scope: seam stitching across UV islands.  (Half-float, RGB9E5 and RGBE output: jpt_encode, below.) */
typedef struct jpt_bake_finish_params {
    int32_t passes;             /* 0..6, default 3: a-trous passes, pass k with tap spacing 2^k; 0 = no filter */
    int32_t normal_power_log2;  /* 0..8, default 4 */
    int32_t dilate;             /* 0..64, default 4: rings of invalid texels filled outwards from the charts */
    float   sigma_distance;     /* finite, > 0, default 4 */
    float   sigma_plane;        /* finite, > 0, default 1 */
    float   sigma_color;        /* finite, > 0, default 4; halves every pass */
} jpt_bake_finish_params;
int jpt_set_bake_finish_params(jpt_ctx *ctx, const jpt_bake_finish_params *params);   /* NULL: the defaults */
int jpt_bake_finish(jpt_ctx *ctx);
int jpt_read_lightmap_f32(jpt_ctx *ctx, float *out);       /* W*H*4 floats: (r, g, b, coverage) */

/* ---- directional lightmaps: the first moments of the incoming light per texel (no reference counterpart; the other half of Godot's
 * LightmapGI with `directional` on, which lets a normal-mapped surface lit by the lightmap keep its relief) ----
 * With the switch on a bake render keeps, beside the sum of a texel's frames, three more sums:
 *     M_k.c  =  sum over the frames f, in frame order, of  cur_f.c * d_f.k          k = world x, y, z;   c = r, g, b
 * cur_f the frame's value exactly as the accumulation adds it (in JPT_ACCUM_REF_LDR8 the rgba8 value read back) and d_f the direction
 * in which the texel's path of frame f left the surface, not renormalised.  Each term is one binary32 multiply and one add, in the
 * accumulation's order; the first render after jpt_accum_reset overwrites; an invalid texel holds +0 in all nine values (DESIGN.md
 * section 2; gdpathtracing_amd/csrc/jpt_bake_dir.h; tests/np_bake_dir.py restates it bit for bit).  M_k / frame_count estimates
 * (1 / pi) * integral of L(w) w_k cos(theta) dw: the first moment of what accum / frame_count is the zeroth moment of.  No SH constant
 * is folded in (INTEGRATION.md has the mapping to L1 coefficients).
 *
 * One kernel of its own, launched behind the accumulation of every bake render on the default kernel; no path kernel differs, and with
 * the switch off no launch, argument or allocation of any render differs.  The switch has no effect on a render without bake images.
 * jpt_set_bake_directional     a CHANGE of the value resets the accumulation as jpt_accum_reset does.  The planes, 48 B per texel of the
 *                              context's rows, exist only while the switch is on and bake images are present.
 * jpt_read_bake_directional_f32  3 * width * local_rows * 4 floats of raw sums: plane k at k * width * local_rows texels, (M_k.r, M_k.g,
 *                              M_k.b, 0) per texel, the context's own rows in their local order.  Waits for the renders queued so far.
 * jpt_device_bake_directional  the device pointer of the raw (finished == 0) or the finished planes and their size; NULL and 0 bytes
 *                              when there are none.
 * jpt_bake_finish_directional  jpt_bake_finish's filter and dilation, once per plane: the plane is the accumulation, the frame count,
 *                              the bake images and jpt_set_bake_finish_params' parameters are the same.  The planes are filtered
 *                              independently of one another and of the L0 map, as Godot denoises its layers.  Guides, working images
 *                              and results of its own, 112 B per texel, kept and freed as jpt_bake_finish's.
 * jpt_read_lightmap_directional_f32  3 * W * H * 4 floats: plane k holds (x, y, z of M_k's filtered mean read as r, g, b; coverage).
 * JPT_E_STATE, with a message naming jpt_set_bake_directional: a render with the switch on and bake images present under
 * JPT_KERNEL_REFERENCE_LAYOUT (it adds frame by frame and keeps no per-frame values), a denoising mode other than
 * JPT_DENOISE_PROGRESSIVE, or jpt_set_debug_steps.  jpt_read_bake_directional_f32: JPT_E_STATE with the switch off, without bake images or
 * before a bake render with the switch on.  jpt_bake_finish_directional: jpt_bake_finish's refusals, and the switch off.
 * jpt_read_lightmap_directional_f32 before a jpt_bake_finish_directional at the current size and images: JPT_E_STATE.  Host-only contexts:
 * JPT_E_DEVICE.  There is no jpt_multi_* form.
 * Not covered: the reference-layout kernel, jpt_multi, encoded output (jpt_encode has no source for the planes), joint filtering with
 * the L0 map, SH above band 1. */
int jpt_set_bake_directional(jpt_ctx *ctx, int32_t enable);
int jpt_read_bake_directional_f32(jpt_ctx *ctx, float *out);
void *jpt_device_bake_directional(jpt_ctx *ctx, int32_t finished, size_t *bytes_out);
int jpt_bake_finish_directional(jpt_ctx *ctx);
int jpt_read_lightmap_directional_f32(jpt_ctx *ctx, float *out);

/* ---- light probes: a sphere tile per probe, projected to L2 spherical harmonics on the device (no reference counterpart; the probes
 * of Godot's LightmapGI that light dynamic objects) ----
 * With probes present every render is a PROBE render: the image holds one tile_w x tile_h tile per probe, side by side, and one render
 * captures them all.  Probe p owns the tile whose top-left pixel is ((p % probes_per_row) * tile_w, (p / probes_per_row) * tile_h); the
 * image is probes_per_row * tile_w wide and ceil(n_probes / probes_per_row) * tile_h high (jpt_get_probe_image_size) -- the size to
 * give jpt_set_params.  A pixel of a tile with index >= n_probes has no path: radiance 0, first-hit distance far, no ray counted, like
 * an invalid bake texel.  Nothing downstream of ray generation knows: both kernels, the environment map and both sampling modes,
 * emitter sampling, glass, the partition, jpt_multi (jpt_set_probes on every rank's jpt_multi_ctx), the read-backs, jpt_display and
 * jpt_meter work on a probe render as on a picture.
 * The ray of cell (i, j) of a tile, frame f (pinned; gdpathtracing_amd/csrc/jpt_probe.h; tests/np_probe.py): the
 * seeds and the jitter draw of a camera ray, taken and discarded; (xi0, xi1) from one pcg2d round of a copy of the seeds hashed with
 * (0x510e527f, 0x9b05688c);
 *     u = (i + xi0) / tile_w, v = (j + xi1) / tile_h, phi = (u - 0.5) * 6.2831853, z = 1 - 2 v, r = sqrt(1 - z z),
 *     d = (r sin phi, z, r cos phi)   in world axes, not renormalised;   o = the probe's position, no offset.
 * This is the cylindrical equal-area map: every cell subtends 4 pi / (tile_w * tile_h).  The polar axis is world +Y, row 0 is the up
 * pole and the centre column is +Z: the orientation of JPT_CAMERA_EQUIRECT with an identity basis.
 * Limits: tile_w in 4..64, tile_h in 2..32, tile_w * tile_h <= 1024, probes_per_row >= 1, a non-finite position: JPT_E_INVALID;
 * n_probes in 1..2^20 and at most 2^26 pixels of image: JPT_E_LIMIT; host-only contexts: JPT_E_DEVICE after these checks.
 * jpt_set_probes WAITS for the renders the context has queued, as jpt_set_bake_texels does; (NULL, 0, 0, 0, 0) frees the probes, after
 * which a render is bit for bit that of a context that never held any.  The positions belong to the context: they survive scene
 * changes, and jpt_scene_share does not copy them.  jpt_read_probes returns them (n_probes * 3 floats).
 * The render calls return JPT_E_STATE, with a message, while probes are present and their image size is not jpt_set_params' width x
 * height, the lens radius is > 0, the camera model is not JPT_CAMERA_PINHOLE or the denoising mode is JPT_DENOISE_TEMPORAL; with bake
 * images also present the render is a bake render (and refused as one).  jpt_set_debug_steps ignores the probes.  jpt_denoise,
 * jpt_query_pixels and jpt_bake_finish return JPT_E_STATE while probes are present: their rays are camera rays or texel images.
 *
 * jpt_probe_project reduces every tile of the accumulation to nine SH coefficients per colour channel, as an explicit call like
 * jpt_bake_finish: enqueued on the context's stream, it READS the accumulation and the frame count and writes only its own buffer, 144
 * B per probe, which jpt_read_probe_sh_f32 returns: n_probes * 9 * 4 floats, (r, g, b, 0) per coefficient.
 * Basis: real SH of bands 0..2 in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), in the frame of the map
 * (X, Y, Z) = (d.z, d.x, d.y) -- Z the polar axis (world +Y), the azimuth from X (world +Z) towards Y (world +X):
 *     Y0 = 0.2820948          Y1 = 0.4886025 d.x       Y2 = 0.4886025 d.y                 Y3 = 0.4886025 d.z
 *     Y4 = 1.0925484 d.z d.x  Y5 = 1.0925484 d.x d.y   Y6 = 0.3153916 (3 d.y d.y - 1)     Y7 = 1.0925484 d.z d.y
 *     Y8 = 0.5462742 (d.z d.z - d.x d.x)
 * Quadrature: a table made on the host in double -- the MEAN of each basis function over each cell (closed forms), times the cell's
 * solid angle, divided by the Gram diagonal sum_cells w mean_k^2 (the off-diagonal terms vanish by symmetry), so constant radiance
 * gives exactly zero above coefficient 0 and any band-limited radiance is recovered exactly from its cell means.  A function whose
 * cell means all vanish on the grid cannot be resolved and its coefficient is 0: Y6 with tile_h = 2, Y8 with tile_w = 4.  With
 * JPT_PROBE_IRRADIANCE band l is multiplied by pi, 2 pi / 3, pi / 4: the coefficients of the irradiance as a function of the normal.
 * The sum is pinned: mean = accum.rgb / frame_count; one wave per probe, lane l adds mean * t (a multiply, then an add) for the cells
 * l, l + 64, ... in raster order into accumulators starting at +0; six butterfly steps v + v[lane ^ s], s = 32 .. 1.
 * JPT_E_STATE, with a message naming the call: no probes; their image size is not jpt_set_params'; no frame accumulated since the
 * last reset; a denoising mode other than JPT_DENOISE_PROGRESSIVE; DEBUG_STEPS mode; a screen partition (the gathering context
 * projects, as with jpt_display).  jpt_read_probe_sh_f32 before a jpt_probe_project of the current probes and size: JPT_E_STATE.
 * Unknown flags: JPT_E_INVALID.  There is no jpt_multi_* form.
 * Out of scope: probe placement and detection of probes inside geometry (jpt_query_rays answers
 * that), band 3 and above, octahedral tiles.  (Cube captures: jpt_set_reflection_probes, below; half-float output: jpt_encode, below.) */
enum { JPT_PROBE_RADIANCE = 0, JPT_PROBE_IRRADIANCE = 1 };
int jpt_set_probes(jpt_ctx *ctx, const float *position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row);
int jpt_get_probe_image_size(jpt_ctx *ctx, int32_t *width, int32_t *height);
int jpt_read_probes(jpt_ctx *ctx, float *position3);       /* what the context holds: n_probes * 3 floats */
int jpt_probe_project(jpt_ctx *ctx, int32_t flags);
int jpt_read_probe_sh_f32(jpt_ctx *ctx, float *out);       /* n_probes * 9 * 4 floats: (r, g, b, 0) per coefficient */

/* ---- reflection probes: a cube capture per probe and a GGX-prefiltered mip chain made on the device (no reference counterpart; the
 * ReflectionProbe that glossy and dynamic objects of a baked Godot scene read) ----
 * With reflection probes present every render is a CUBE render.  With S = face_size, probe p owns the strip 6 S wide and S high whose
 * top-left pixel is ((p % probes_per_row) * 6 S, (p / probes_per_row) * S); face f of the strip is the S x S square at x = f * S.  The
 * image is probes_per_row * 6 S wide and ceil(n_probes / probes_per_row) * S high (jpt_get_reflection_image_size) -- the size to give
 * jpt_set_params.  A pixel of a strip with index >= n_probes has no path: radiance 0, first-hit distance far, no ray counted, like a
 * tile without a light probe.  Nothing downstream of ray generation knows: both kernels, the environment map and both sampling modes,
 * emitter sampling, glass, the partition, the read-backs, jpt_display and jpt_meter work on a cube render as on a picture.
 * The ray of texel (i, j) of face f, frame n (pinned; gdpathtracing_amd/csrc/jpt_cube.h; tests/np_reflection.py):
 * the seeds and the jitter draw of a camera ray, taken and discarded; (xi0, xi1) from one pcg2d round of a copy of the seeds hashed
 * with (0x1f83d9ab, 0x5be0cd19);
 *     a = 2 ((i + xi0) / S) - 1,  b = 2 ((j + xi1) / S) - 1,  d = normalize3 of the OpenGL cube-map face table (Godot's):
 *     face 0 = +X ( 1, -b, -a)   face 1 = -X (-1, -b,  a)   face 2 = +Y ( a,  1,  b)
 *     face 3 = -Y ( a, -1, -b)   face 4 = +Z ( a, -b,  1)   face 5 = -Z (-a, -b, -1);        o = the probe's position, no offset.
 * A texel's accumulated mean is thus its box-filtered radiance in face coordinates.
 * Limits: face_size a power of two in 4..256, probes_per_row >= 1, a non-finite position: JPT_E_INVALID; n_probes in 1..2^20 and at
 * most 2^26 pixels of image: JPT_E_LIMIT; host-only contexts: JPT_E_DEVICE after these checks.
 * jpt_set_reflection_probes WAITS for the renders the context has queued, as jpt_set_probes does; (NULL, 0, 0, 0) frees the probes and
 * the chain, after which a render is bit for bit that of a context that never held any.  The positions belong to the context: they
 * survive scene changes, and jpt_scene_share does not copy them.  jpt_read_reflection_probes returns them (n_probes * 3 floats).
 * The render calls return JPT_E_STATE, with a message, while reflection probes are present and the context also holds light probes
 * (jpt_set_probes) or bake images, their image size is not jpt_set_params' width x height, the lens radius is > 0, the camera model
 * is not JPT_CAMERA_PINHOLE or the denoising mode is JPT_DENOISE_TEMPORAL.  jpt_set_debug_steps ignores the probes.  jpt_denoise,
 * jpt_query_pixels, jpt_bake_finish and jpt_probe_project return JPT_E_STATE while reflection probes are present.
 *
 * jpt_reflection_prefilter makes the mip chain, as an explicit call like jpt_probe_project: enqueued on the context's stream, it READS
 * the accumulation and the frame count and writes only its own images; every render, buffer and read-back is bit for bit what it is
 * without the call.  Level l of the chain has faces of s_l = S >> l texels and holds the radiance convolved with the GGX lobe of
 * roughness l / (n_levels - 1): a material of roughness r reads mip r * (n_levels - 1).  The radiance is linear and not pre-multiplied
 * by any BRDF term.  jpt_read_reflection_f32 returns one level: n_probes * 6 * s_l^2 float4 (r, g, b, 1), probe-major, then face,
 * row, column; jpt_get_reflection_chain_size gives s_l and where the level starts in the chain, in texels (n_probes * 8 (S^2 - s_l^2)).
 * jpt_set_reflection_params: n_levels in 2..log2(S) + 1, or 0 for every level down to 1 x 1 (the default); samples (K) in 8..256,
 * default 64; NULL: the defaults; anything else JPT_E_INVALID (n_levels is checked against the probes the context holds then, and again
 * by jpt_reflection_prefilter: JPT_E_STATE).
 * Arithmetic (pinned; gdpathtracing_amd/csrc/jpt_reflection.h):
 *   source chain per probe and face: level 0 = accum.rgb / (float)frame_count; level m + 1 = ((a + b) + (c + d)) * 0.25 of the 2 x 2
 *     block, down to 1 x 1;
 *   output level 0 = source level 0 with alpha 1; level l >= 1: alpha = l / (n_levels - 1) (the renderer's convention: roughness^2 is
 *     alpha^2; the standard GGX NDF), a table of K samples made on the host in double: u1 = (k + 0.5) / K, u2 the base-2 radical
 *     inverse of k, cos t = sqrt((1 - u1) / (1 + (alpha^2 - 1) u1)), phi = 2 pi u2, h = (sin t cos phi, sin t sin phi, cos t), L = (2 h_z
 *     h_x, 2 h_z h_y, 2 h_z^2 - 1) (view = normal = the texel's direction); samples with L_z <= 0 are dropped; w = L_z / sum L_z; the
 *     sample reads source level clamp(floor(0.5 log2(O_s / O_0) + 0.5) + 1, 0, log2 S) with O_s = 4 / (K D(h_z)), O_0 = 4 pi / (6 S^2);
 *   output texel (f, i, j) of a level of size s: N = normalize3(face table at a = (2 (i + 0.5)) / s - 1, b likewise); the branch-free
 *     tangent frame of Duff et al.; d = (T L_x + B L_y) + N L_z; the nearest texel of the source level in direction d (major axis by
 *     |x| >= |y| && |x| >= |z|, else |y| >= |z|, else z); acc = acc + c * w_k for k ascending, from +0.
 * JPT_E_STATE, with a message naming the call: no reflection probes; light probes or bake images beside them; their image size is not
 * jpt_set_params'; no frame accumulated since the last reset; a denoising mode other than JPT_DENOISE_PROGRESSIVE; DEBUG_STEPS mode; a
 * screen partition.  jpt_read_reflection_f32 before a jpt_reflection_prefilter of the current probes, size and parameters: JPT_E_STATE.
 * jpt_get_reflection_timing: the kernel time of the last jpt_reflection_prefilter's two steps (the source chain, the prefilter) in ms,
 * when it ran under jpt_set_kernel_timing (else JPT_E_STATE); it waits for them.
 * Out of scope: box projection / parallax correction, blending between probes, bilinear or cross-face filtering of the source, the
 * BRDF split-sum LUT, an octahedral layout, a jpt_multi_* form, anisotropy, any change to how materials are shaded.  (Half-float,
 * RGB9E5 and RGBE output: jpt_encode, below.) */
typedef struct { int32_t n_levels; int32_t samples; } jpt_reflection_params;   /* defaults: every level down to 1x1 (0); 64 */
int jpt_set_reflection_probes(jpt_ctx *ctx, const float *position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row);
int jpt_get_reflection_image_size(jpt_ctx *ctx, int32_t *width, int32_t *height);
int jpt_read_reflection_probes(jpt_ctx *ctx, float *position3);   /* what the context holds: n_probes * 3 floats */
int jpt_set_reflection_params(jpt_ctx *ctx, const jpt_reflection_params *params);   /* NULL: the defaults */
int jpt_reflection_prefilter(jpt_ctx *ctx);
int jpt_get_reflection_chain_size(jpt_ctx *ctx, int32_t level, int32_t *face_size, uint64_t *offset_texels);
int jpt_read_reflection_f32(jpt_ctx *ctx, int32_t level, float *out);   /* n_probes * 6 * s_l^2 float4 (r, g, b, 1), s_l = S >> level */
int jpt_get_reflection_timing(jpt_ctx *ctx, float *chain_ms, float *prefilter_ms);

/* Which device pipeline renders (no reference counterpart; both give the same image):
 *   WAVEFRONT          queue-based path tracer over the flattened 64-byte-node layout (default, fast);
 *   REFERENCE_LAYOUT   one thread per pixel straight over the six reference-layout buffers, node for node
 *                      as main.glsl:270-350 (audit route). */
enum { JPT_KERNEL_WAVEFRONT = 0, JPT_KERNEL_REFERENCE_LAYOUT = 1 };
int jpt_set_kernel(jpt_ctx *ctx, int32_t variant);

/* replaces: building main.glsl with `#define DEBUG_STEPS` (main.glsl:4, commented out as shipped; the reference's one
 * verification aid): every frame's image is clamp(hitInfo.steps / 256) in all three channels -- the number of
 * intersectTriangle calls the PRIMARY ray made (main.glsl:225,358-361,423-427) --, one ray per pixel, depth = far; the
 * post-processing pass runs on it as on any frame.  Rendered by the audit kernel (whatever jpt_set_kernel says), which
 * walks the scene's tree in reference layout: on the reference's own tree (JPT_UPLOAD_WALK_AS_GIVEN uploads,
 * JPT_BUILD_REFERENCE_EXACT commits) the counts are the reference's, on a native tree they are that tree's. */
int jpt_set_debug_steps(jpt_ctx *ctx, int32_t enable);

/* Per-launch timing of the traversal kernels (HIP events recorded around each launch on the context's stream;
 * jpt_stats.last_trace_ms).  Off by default: each event costs a few microseconds between kernels. */
int jpt_set_kernel_timing(jpt_ctx *ctx, int32_t enable);

/* Multi-GPU screen partition (no reference counterpart): this context renders the
 * 8-row strips s with s % world == rank.  Default rank 0 of 1 = whole image. */
int jpt_set_partition(jpt_ctx *ctx, int32_t rank, int32_t world);

/* replaces: cs->update_storage_buffer_uniform(camera_rid, camera.to_packed_byte_array())
 * (path_tracing_camera.cpp:198-200).  camera160 = struct Camera (render_parameters.h:14-21); its
 * frame_index field is ignored -- jpt_render takes the frame index explicitly. */
int jpt_set_camera(jpt_ctx *ctx, const void *camera160);

/* replaces n_frames iterations of PathTracingCamera::render's GPU work: cs->compute(main.glsl)
 * + ProgressiveRendering::render (path_tracing_camera.cpp:199-214, progressive_rendering.cpp:53-65).
 * Frame f uses camera.frame_index = first_frame_index + f and continues the accumulation
 * (frame_count = frames since jpt_accum_reset).  Blocking; device time in jpt_stats. */
int jpt_render(jpt_ctx *ctx, int32_t n_frames, uint32_t first_frame_index);
/* Same result, kernels compiled with event counters; fills the jpt_stats counter fields. */
int jpt_render_counted(jpt_ctx *ctx, int32_t n_frames, uint32_t first_frame_index);
/* Asynchronous form: enqueue and return; jpt_sync() or a jpt_read_* waits.  Consecutive asynchronous renders are
 * pipelined: their kernels run on alternating internal streams with separate workspaces (one render's launch
 * tails overlap the next render's kernels), the accumulation kernels run in call order (chained by events through
 * the ctx stream, which waits for each of them: work queued on the ctx stream afterwards sees the result), so the
 * framebuffers hold exactly what serial execution would leave (C3: 1.78 -> 1.28 ms per render when queued; up to four
 * renders are in flight, each with its own workspace).  A host that keeps only ONE render in flight (enqueue, own work,
 * jpt_sync or a read, enqueue ...) is recognised after its third such render and served like jpt_render from then on
 * (the pipelined launches are narrow: alone they take half as long again), still without blocking the caller. */
int jpt_render_async(jpt_ctx *ctx, int32_t n_frames, uint32_t first_frame_index);
int jpt_sync(jpt_ctx *ctx);

/* replaces: camera_moved -> frame_count = 1 (progressive_rendering.cpp:53-57).  In temporal mode: the history
 * images start from zero again, as for a newly created TemporalReprojection (temporal_reprojection.cpp:42-43), and
 * jpt_read_accum_f32 answers JPT_E_STATE until the next pass has written one.  A change of mode and jpt_set_params with
 * another width or height do the same. */
int jpt_accum_reset(jpt_ctx *ctx);
/* replaces: the frame_count word of ProgressiveRendering's Params (progressive_rendering.cpp:53-61, read at
 * progressive_rendering.glsl:34,39), for hosts that keep that counter themselves (the gdcs-shaped adapter hands over
 * what the reference's own ProgressiveRendering::render computed).  The next frame rendered is accumulated as frame
 * number `next_frame_count`: 1 overwrites the float sum (what jpt_accum_reset arranges), n > 1 adds to whatever the
 * buffer holds -- zeros after jpt_set_params, like the reference's freshly created frameBuffer image -- and the screen
 * is ACES(sum / n).  (The reference's very first frame has n = 2 when the camera's transform is the identity:
 * previous_transform starts as the identity, so camera_moved is false.) */
int jpt_set_progressive_frame_count(jpt_ctx *ctx, uint32_t next_frame_count);

/* replaces: the denoising_mode switch of PathTracingCamera::render (path_tracing_camera.cpp:207-225).
 *   JPT_DENOISE_PROGRESSIVE (default)  as described above.
 *   JPT_DENOISE_NONE       the screen (jpt_read_ldr_rgba8) is the rgba8 image main.glsl stored for the LAST frame
 *                          of the call, no tone mapping (path_tracing_camera.cpp:222-224).
 *   JPT_DENOISE_TEMPORAL   jpt_render takes n_frames = 1: trace the frame, then one dispatch of
 *                          temporal_reprojection.glsl with the parameters of jpt_set_temporal_params: the screen is
 *                          ACES(mix(frame, reprojected history, 0.75)); jpt_read_accum_f32 returns the rgba32f
 *                          history image that dispatch wrote.  Whole image on one context (no partition).
 * Changing the mode restarts the accumulation / history. */
int jpt_set_denoising_mode(jpt_ctx *ctx, int32_t mode);
/* replaces: cs->update_storage_buffer_uniform(render_parameters_rid, ...) of TemporalReprojection::render
 * (temporal_reprojection.cpp:67): the 88-byte TemporalReprojection::RenderParameters (temporal_reprojection.h:16-23:
 * deltaMatrix[16] column-major, width, height, frame_count, blendFactor, nearPlane, farPlane).  frame_count picks
 * the history image to read (even: frameBuffer1) and to write; blendFactor is not read by the shader
 * (temporal_reprojection.glsl:64 uses the literal 0.75) and is not read here. */
int jpt_set_temporal_params(jpt_ctx *ctx, const void *render_parameters88);

/* Which of main.glsl's two images a render produces (ABI 5).  The reference stores both every frame (main.glsl:434-435), but its
 * r32f depth image has one reader, TemporalReprojection (temporal_reprojection.glsl:45-58; add_existing_buffer at
 * temporal_reprojection.cpp:33): in the progressive and "none" modes nothing ever looks at it ("result-
 * preserving freedoms").  JPT_OUTPUT_DEPTH off: the kernels neither keep the first-hit distances nor write the depth image
 * (8.3 MB per 1080p render), and jpt_read_depth_f32 answers JPT_E_STATE.  Default: on, as the reference; JPT_DENOISE_TEMPORAL
 * renders produce it whatever this says.  The colour image, the accumulation and the display image are not affected. */
enum { JPT_OUTPUT_DEPTH = 1 };
int jpt_set_outputs(jpt_ctx *ctx, uint32_t outputs);

/* ---- spatial denoising of the accumulation (no reference counterpart; the reference lists a denoiser among its wanted features) --
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the running mean of the progressive accumulation, guided by
 * first-hit position, normal and albedo images, as an explicit call: nothing runs unless the host asks, and without jpt_denoise
 * every render, buffer and read-back is exactly what it is without this section.  The arithmetic is pinned in DESIGN.md section 2
 * (gdpathtracing_amd/csrc/jpt_denoise.h; tests/np_denoise.py restates it bit for bit).
 *
 * jpt_denoise enqueues, on the context's stream, behind every render queued before it and ahead of those queued after it:
 *   the guide pass   one un-jittered primary ray per pixel centre, with the camera, scene and sampler mode current at the call, over
 *                    the arrays the wavefront kernels walk (whatever jpt_set_kernel says; it follows jpt_scene_refit_tlas and
 *                    jpt_scene_update_mesh).  Closest hit = the smallest accepted Moller-Trumbore t, no reach or tie logic.
 *                    position_t = (position, distance from the camera), normal = (shading normal, 0), albedo = (diffuse albedo +
 *                    fresnel_0, 0), or (1, 1, 1, 0) on an emitter; a miss: (0, 0, 0, -1), 0, (1, 1, 1, 0).
 *   `passes` filter passes, pass k with tap spacing 2^k, over (accum / frame_count) / max(albedo, 1/64), then the product with
 *                    that albedo again (the denoised image, linear) and its display image unorm8(ACES(.)).
 * It READS the accumulation and the frame count and writes only its own images (3 guides, 2 colour images, one rgba8 image: 84
 * bytes per pixel, allocated at the first call at a resolution, freed by jpt_set_params with another size and by jpt_destroy):
 * jpt_read_accum_f32 / _ldr_rgba8 / _depth_f32, the split read-back and every later render are bit for bit what they are without
 * the call -- the accumulation goes on unbiased underneath, the denoised image is a view of it.
 * JPT_E_STATE: no scene; no frame accumulated since the last reset; a denoising mode other than JPT_DENOISE_PROGRESSIVE; the
 * DEBUG_STEPS mode; a screen partition (whole image on one context, as JPT_DENOISE_TEMPORAL); jpt_read_denoised_* /
 * jpt_read_guides_f32 before a jpt_denoise at the current resolution.  Host-only contexts: JPT_E_DEVICE.
 * The parameters are the context's (like jpt_set_params'): they survive scene changes, each jpt_denoise takes them by value,
 * jpt_scene_share does not copy them.  JPT_E_INVALID outside the ranges below or for a non-finite sigma. */
typedef struct jpt_denoise_params {
    int32_t passes;             /* 1..6, default 5: pass k uses tap spacing 2^k */
    int32_t normal_power_log2;  /* 0..8, default 6: the normal weight max(0, n.n') is squared this many times */
    float   sigma_plane;        /* > 0, default 0.02: tolerated distance from the centre's tangent plane, relative to its hit distance */
    float   sigma_color;        /* > 0, default 4.0: colour tolerance in units of the demodulated mean; halves every pass */
} jpt_denoise_params;
int jpt_set_denoise_params(jpt_ctx *ctx, const jpt_denoise_params *params);   /* NULL: the defaults */
int jpt_denoise(jpt_ctx *ctx);
/* The read-backs wait for the work queued on the context, through its pinned staging buffer like the other jpt_read_*. */
int jpt_read_denoised_f32(jpt_ctx *ctx, float *out);       /* W*H*4 floats (r, g, b, 1), linear */
int jpt_read_denoised_rgba8(jpt_ctx *ctx, uint8_t *out);   /* W*H*4 bytes: unorm8(ACES(denoised)), alpha 255 */
int jpt_read_guides_f32(jpt_ctx *ctx, float *position_t, float *normal, float *albedo);   /* each W*H*4 floats, or NULL */

/* ---- variance guidance of jpt_denoise (no reference counterpart; the colour weight of SVGF, Schied et al. 2017) ------------------
 * A fixed colour tolerance cannot tell noise from signal: it blurs a shadow edge on a flat wall, where no guide has an edge, and it
 * biases an image that is already clean.  With the guidance on, jpt_denoise measures colour differences against the variance of the
 * mean, from the plane of jpt_set_variance (below), instead of against sigma_color.  Off, the default, jpt_denoise launches what it
 * launches without this section, and every output is bit for bit the same.  The arithmetic is pinned in DESIGN.md section 2
 * (gdpathtracing_amd/csrc/jpt_denoise_var.h; tests/np_denoise_var.py restates it bit for bit); every operation is one binary32
 * operation in the order written.  With nf = (float)frame_count, q = nf * (nf - 1), a = max(albedo, 1/64) per channel:
 *   first       i_0 = (accum / nf) / a;  v_0 = m2.r / q / (a.r * a.r) + m2.g / q / (a.g * a.g) + m2.b / q / (a.b * a.b), left to right; a
 *               v_0 that is not finite or not > 0 is +0.  It is the variance of the demodulated mean summed over the channels, as
 *               |dc|^2 below is a sum over the channels.  Pass k carries (i_k, v_k).
 *   per pass    gv = the 3 x 3 binomial (1 2 1)/4 x (1 2 1)/4 of v_k around the pixel, tap spacing 1 in every pass, over the taps
 *               inside the image, divided by the sum of the weights used;  den = (sigma_variance * sigma_variance) * gv +
 *               variance_floor;  the colour weight of tap q is 1 / (1 + |c_q - c_p|^2 / den) -- den is not halved per pass, the
 *               shrinking v_k does that -- and everything else is jpt_denoise's: the geometric weight, the binomial taps and their
 *               order, a tap of weight 0 is not multiplied, the rules for colours that are not finite.
 *               i_k+1 = sum wt c_q / sum wt;  v_k+1 = sum (wt * wt) v_q / (sum wt * sum wt).  A centre whose colour is not finite
 *               keeps its colour and its v.
 *   last        the denoised image (i * a, 1) and its rgba8 image as without the guidance -- jpt_display, jpt_meter and jpt_encode
 *               read them as they read jpt_denoise's -- and v of the last pass in a plane of its own (4 B per pixel, in demodulated
 *               units, allocated by the first guided jpt_denoise at a resolution): jpt_read_denoised_variance_f32.
 * The parameters are the context's, as jpt_set_denoise_params': they survive scene changes and jpt_scene_share does not copy them.
 * JPT_E_INVALID: enable not 0 or 1, a sigma_variance or variance_floor that is not finite or not > 0, reserved != 0.  With the
 * guidance on jpt_denoise answers JPT_E_STATE -- it never falls back to the fixed tolerance -- when the variance plane is switched
 * off (jpt_set_variance), when no render has written it at the current size, and when fewer than two frames are accumulated; it is
 * otherwise ordered on the stream as without the guidance, READS the accumulation, the frame count and the plane and writes only its
 * own images.  jpt_read_denoised_variance_f32: JPT_E_STATE unless the last jpt_denoise at the current resolution was a guided one.
 * Host-only contexts: JPT_E_DEVICE.  Not covered: jpt_bake_finish, a partition or jpt_multi, a jpt_encode source for the variance
 * image, per-channel variance.  (The temporal component is jpt_set_denoise_history, below.) */
typedef struct jpt_denoise_variance_params {
    int32_t enable;          /* 0 or 1, default 0 */
    float   sigma_variance;  /* finite, > 0, default 2.0: colour tolerance in standard deviations of the mean */
    float   variance_floor;  /* finite, > 0, default 1e-6: added to the scaled variance, so that a clean pixel still has a tolerance */
    int32_t reserved;        /* 0 */
} jpt_denoise_variance_params;
int jpt_set_denoise_variance(jpt_ctx *ctx, const jpt_denoise_variance_params *params);   /* NULL: the defaults */
int jpt_read_denoised_variance_f32(jpt_ctx *ctx, float *out);                            /* W*H floats: v of the last pass */

/* ---- history for jpt_denoise: past frames reprojected through the guides (no reference counterpart; the temporal stage of SVGF) ----
 * An interactive viewport renders one sample per pixel per frame under a moving camera (jpt_accum_reset, jpt_render(1), show): the
 * progressive mean never gets past one frame and the variance plane has nothing to measure.  With the history on, each jpt_denoise
 * integrates the mean of the frames accumulated since the last reset into a per-pixel history that follows the surfaces: it is
 * reprojected from the previous call's view, validated against the previous call's position and normal guides, and its variance feeds
 * the variance-guided passes above.  Off, the default, jpt_denoise launches what it launches without this section.  The arithmetic is
 * pinned in DESIGN.md section 2 (gdpathtracing_amd/csrc/jpt_denoise_history.h; tests/np_denoise_history.py restates it bit for bit);
 * every operation is one binary32 operation in the order written.  One call, on the context's stream as jpt_denoise is ordered:
 *   guides      the guide pass, unchanged: X = position_t, n, albedo; a = max(albedo, 1/64)
 *   history     per pixel, nf = (float)frame_count: the sample c = (accum / nf) / a.  A miss or a c that is not finite takes no
 *               history and leaves none (length 0; the filter gets (c, +0)).  Previous view (RefCamera vp and position) bit-identical
 *               to this one: the one tap is the pixel's own previous texel, taken as it is.  Else clip = vp_prev * (X, 1), clip.w > 0,
 *               u = (clip.x / clip.w + 1) / 2 * W, v = (1 - clip.y / clip.w) / 2 * H, and the four bilinear taps around (u - 0.5,
 *               v - 0.5) inside the image.  A tap weighs its bilinear weight times the geometric weight of jpt_denoise (normal_power_log2
 *               of jpt_set_denoise_params, sigma_plane of this struct) of the previous call's position and normal at the tap seen from
 *               this pixel; a tap of history length 0, or whose m or S is not finite, weighs 0.  Sum of weights > 0: m_h, S_h, N_h are the weighted means.
 *               N = max(min(N_h + nf, max_history), nf), al = nf / N, d = c - m_h, m = m_h + al * d, S = (1 - al) * (S_h + al * |d|^2)
 *               (West's update: no raw second moments).  No history: m = c, S = 0, N = nf.
 *               N_h >= min_history: v_0 = S * al / (1 - al), the variance of m summed over the channels -- exactly m2 / (k (k - 1))
 *               while the history grows, twice the steady-state variance once it is capped.  Else the variance of c over the accepted
 *               taps of the pixel's 5 x 5 window (inside the image, finite, geometric weight > 0) times al; fewer than two taps: +0.
 *   filter      the passes of jpt_set_denoise_variance over (m, v_0), with its sigma_variance and variance_floor; neither its enable
 *               nor jpt_set_variance needs to be on.  The outputs are jpt_denoise's: the denoised image, its rgba8 image and the v
 *               plane (jpt_read_denoised_*, jpt_read_denoised_variance_f32, jpt_display, jpt_meter, jpt_encode with DENOISED).
 * A call consumes its frames: a second history call with none of jpt_accum_reset, jpt_set_progressive_frame_count, jpt_set_params
 * (or jpt_set_partition, which re-makes the framebuffers too) and a jpt_set_denoising_mode that changes the mode -- the calls that
 * restart or re-position the accumulation -- in between would count them twice and answers JPT_E_STATE; jpt_denoise_history_reset
 * and switching enable release the frames with the history they were counted in.  With the history on jpt_denoise also answers JPT_E_STATE with a lens
 * radius > 0, a camera model other than JPT_CAMERA_PINHOLE, bake images, probes or reflection probes, beside what it refuses anyway.
 * The history (three planes of 16 B per pixel, twice, and the (m, v_0) image: 112 B per pixel, from the first history call at a
 * resolution) is dropped by jpt_denoise_history_reset, by jpt_set_params with another size, by switching enable and by jpt_destroy --
 * not by scene changes: where a surface moved the geometric test rejects the tap and the pixel starts over (there are no motion
 * vectors).  A jpt_denoise with the history off leaves it untouched.  The parameters are the context's, as jpt_set_denoise_params':
 * they survive scene changes and jpt_scene_share does not copy them.  JPT_E_INVALID: enable not 0 or 1, max_history outside
 * [1, 65536], min_history outside [1, max_history], a sigma_plane that is not finite or not > 0, reserved != 0.  Host-only contexts:
 * JPT_E_DEVICE after the checks that need no device.  Not covered: motion vectors, feedback of the filtered image into the history,
 * a 3 x 3 search when all four taps fail, neighbourhood colour clamping, lens and non-pinhole views, bakes and probes, a partition
 * or jpt_multi, jpt_bake_finish, reprojection of sky pixels. */
typedef struct jpt_denoise_history_params {
    int32_t enable;          /* 0 or 1, default 0 */
    int32_t max_history;     /* 1..65536 frames, default 32: the history length is capped here (an exponential average from then on) */
    int32_t min_history;     /* 1..max_history frames, default 4: below it the variance is the spatial estimate */
    float   sigma_plane;     /* finite, > 0, default 0.05: tolerated distance of a history tap from the pixel's tangent plane, relative to its hit distance */
    int32_t reserved[4];     /* 0 */
} jpt_denoise_history_params;
int jpt_set_denoise_history(jpt_ctx *ctx, const jpt_denoise_history_params *params);   /* NULL: the defaults */
int jpt_denoise_history_reset(jpt_ctx *ctx);                                            /* the next jpt_denoise starts without history */
int jpt_read_denoise_history_f32(jpt_ctx *ctx, float *integrated4, float *length);      /* W*H*4 (m.rgb demodulated, v_0) and W*H floats (N); either may be NULL */

/* ---- the display transform: exposure, bloom, selectable tone mapping (no reference counterpart; the reference lists "simple post
 * processing (e.g. bloom, controllable tone-mapping)" among its wanted features) ------------------------------------------------
 * A graded display image from the progressive accumulation or from jpt_denoise's image, as an explicit call: nothing runs unless
 * the host asks, and without jpt_display every render, buffer and read-back is exactly what it is without this section.  The
 * arithmetic is pinned in DESIGN.md section 2 (gdpathtracing_amd/csrc/jpt_display.h; tests/np_display.py restates it bit for bit):
 *   base        c = (accum / frame_count) * exposure           (JPT_DISPLAY_SOURCE_DENOISED: jpt_denoise's image * exposure)
 *   bloom       (bloom_levels = N > 0) what of c lies over bloom_threshold by luminance (a pixel with a non-finite channel gives
 *               nothing), halved N times with a 4 x 4 binomial filter, summed back up with a 2 x tent filter;
 *               o = c + bloom * (bloom_strength / N)
 *   tone map    JPT_TONEMAP_ACES_REF: the reference's ACES fit; _REINHARD: clamp(o (1 + o / white^2) / (1 + o), 0, 1);
 *               _CLAMP: clamp(o, 0, 1).  A NaN gives 0.
 *   transfer    JPT_TRANSFER_LINEAR: unorm8, as the reference stores; _SRGB: the sRGB code nearest to the encoded value (a search of
 *               the 255 code boundaries jpt_debug_display_srgb_table hands out; IEC 61966-2-1).
 * With the default parameters the rgba8 image equals jpt_read_ldr_rgba8 byte for byte; with source = DENOISED and the rest at the
 * defaults it equals jpt_read_denoised_rgba8.
 *
 * jpt_display enqueues its kernels on the context's stream, ordered as jpt_denoise is: behind every render (and jpt_denoise) queued
 * before it and ahead of those queued after it.  It READS the accumulation and the frame count, or jpt_denoise's image, and writes
 * only its own buffers: the tone-mapped image (16 bytes per pixel) and the encoded image (4 bytes per pixel), allocated at the first
 * call at a resolution, and the bloom pyramid (16 bytes for each of the ~0.34 pyramid pixels per image pixel of six levels: 5.4
 * bytes per pixel), allocated at the first call with bloom_levels > 0 -- 25.4 bytes per pixel in all, freed by jpt_set_params with
 * another size and by jpt_destroy.
 * JPT_E_STATE: a denoising mode other than JPT_DENOISE_PROGRESSIVE; the DEBUG_STEPS mode; a screen partition (the bloom reads rows
 * the context does not hold); jpt_set_params not called; no frame accumulated since the last reset; source = DENOISED without a
 * jpt_denoise at the current resolution; jpt_read_display_* before a jpt_display at the current resolution.  Host-only contexts:
 * JPT_E_DEVICE, after the checks that need no device.
 * The parameters are the context's: they survive scene changes, each jpt_display takes them by value, jpt_scene_share does not copy
 * them.  JPT_E_INVALID outside the ranges below or for a non-finite value. */
enum { JPT_DISPLAY_SOURCE_ACCUM = 0, JPT_DISPLAY_SOURCE_DENOISED = 1 };
enum { JPT_TONEMAP_ACES_REF = 0, JPT_TONEMAP_REINHARD = 1, JPT_TONEMAP_CLAMP = 2 };
enum { JPT_TRANSFER_LINEAR = 0, JPT_TRANSFER_SRGB = 1 };
typedef struct jpt_display_params {
    int32_t source;          /* default JPT_DISPLAY_SOURCE_ACCUM */
    int32_t tonemap;         /* default JPT_TONEMAP_ACES_REF: progressive_rendering.glsl:19-26 */
    int32_t transfer;        /* default JPT_TRANSFER_LINEAR: what the reference stores */
    int32_t bloom_levels;    /* 0..6, default 0 = no bloom */
    float   exposure;        /* finite, >= 0, default 1 */
    float   white;           /* JPT_TONEMAP_REINHARD's white point, finite, > 0, default 4 */
    float   bloom_threshold; /* finite, >= 0, default 1 */
    float   bloom_strength;  /* finite, >= 0, default 0.25 */
} jpt_display_params;
int jpt_set_display_params(jpt_ctx *ctx, const jpt_display_params *params);   /* NULL: the defaults */
int jpt_display(jpt_ctx *ctx);
/* The read-backs wait for the work queued on the context, through its pinned staging buffer like the other jpt_read_*. */
int jpt_read_display_rgba8(jpt_ctx *ctx, uint8_t *out);   /* W*H*4 bytes, alpha 255 */
int jpt_read_display_f32(jpt_ctx *ctx, float *out);       /* W*H*4 floats: the tone-mapped value before the transfer, (r, g, b, 1) */

/* ---- encoded outputs: half-float, RGB9E5 and RGBE read-backs made on the device (no reference counterpart: the reference hands its
 * images to the engine as float4) ------------------------------------------------------------------------------------------------------
 * Every image the library makes on the device is 16 bytes per texel; an engine stores none of them so (a Godot lightmap or panorama is
 * Image.FORMAT_RGBE9995 or FORMAT_RGBAH, a reflection atlas and an HDR viewport texture are half float, an environment map on disk is a
 * Radiance .hdr: INTEGRATION.md).  jpt_encode packs one of those images into such a format on the device, so that 8 or 4 bytes per texel
 * cross the bus instead of 16.  An explicit call: without it every render, buffer and read-back is bit for bit what it is without this
 * section.
 *   source        what is read (always float4)                                                                       texels
 *   MEAN          the accumulation: rgb / (float)frame_count, one IEEE division per channel; alpha written as 1       W x H
 *   DENOISED      what jpt_read_denoised_f32 reads                                                                   W x H
 *   DISPLAY       what jpt_read_display_f32 reads                                                                    W x H
 *   LIGHTMAP      what jpt_read_lightmap_f32 reads (alpha is coverage: 0, 0.5 and 1 are exact in half)                W x H
 *   REFLECTION    level >= 0: that level as jpt_read_reflection_f32 lays it out; JPT_ENCODE_ALL_LEVELS: the whole chain, level l
 *                 starting at offset_texels(l) * bytes per texel (jpt_get_reflection_chain_size)
 *   PROBE_SH      what jpt_read_probe_sh_f32 reads: n_probes * 9 texels, in the tile-frame order.  Signed: JPT_ENCODE_RGBA16F only
 * `level` must be 0 for every source but REFLECTION.  Each source refuses with the code and the words of its own read-back when its
 * image is not there (JPT_E_STATE); MEAN refuses what jpt_display refuses: a denoising mode other than JPT_DENOISE_PROGRESSIVE, the
 * DEBUG_STEPS mode, a screen partition, jpt_set_params not called, no frame accumulated since the last reset.  An unknown source or
 * format, PROBE_SH with another format than RGBA16F, a level that is not there: JPT_E_INVALID.  Host-only contexts: JPT_E_DEVICE after
 * the argument checks.  There is no jpt_multi_* form.
 * The formats (pinned; gdpathtracing_amd/csrc/jpt_encode.h; tests/np_encode.py restates them bit for bit):
 *   RGBA16F   8 B per texel, r g b a in ascending addresses.  Per channel NaN -> +0, clamp to [-65504, 65504] (so +-inf saturate), round
 *             to nearest even; subnormal halves are kept and -0 stays -0.
 *   RGB9E5    4 B per texel, r | g << 9 | b << 18 | e << 27 (VK_FORMAT_E5B9G9R9_UFLOAT_PACK32, GL_RGB9_E5); alpha is dropped.  Per
 *             channel NaN -> 0, clamp to [0, 65408]; e and the mantissas as the extension's specification rounds them.  A channel decodes
 *             as mantissa * 2^(e - 24), within (0.5 + 2^-16) * 2^(e - 24) of the clamped value.
 *   RGBE8     4 B per texel, Ward's r g b mantissas and exponent byte in ascending addresses (a Radiance .hdr file's texels); alpha is
 *             dropped.  Per channel NaN -> 0, clamp to [0, the largest float below 2^127]; mantissas truncated, as float2rgbe does; a
 *             texel whose largest channel is below 1e-32f is four zero bytes.
 * jpt_encode enqueues one kernel on the context's stream, ordered as jpt_display is: behind everything queued before it and ahead of
 * everything queued after it.  It reads its source and writes a buffer of its own (grown when needed, freed by jpt_destroy), which is
 * a SNAPSHOT: it stays readable, with its jpt_encoded_info, until the next jpt_encode or jpt_destroy, whatever happens to the context
 * in between (jpt_set_params with another size included).  jpt_encoded_info: width x height are W x H for the flat sources, the face
 * size of the level (of level 0 for the whole chain) for REFLECTION, and 9 x n_probes for PROBE_SH; n_texels and bytes are the whole
 * buffer's.
 * jpt_read_encoded waits for the work queued on the context and copies through the pinned staging buffer of the other jpt_read_*;
 * jpt_readback_encoded_begin / _end are its split form, as jpt_readback_ldr_begin / _end, with a pinned buffer, an event and a pending
 * flag of their own: begin while one is pending is JPT_E_STATE, end without one too; a jpt_encode while one is pending is legal (the
 * copy was queued first).  `capacity` below the encoded size: JPT_E_INVALID (a pending read-back stays pending).  Before any jpt_encode:
 * JPT_E_STATE.  jpt_device_encoded: the buffer's device pointer and size (NULL and 0 before any jpt_encode), for interop without the
 * host; work that reads it must be ordered behind the context's stream.  jpt_get_encode_timing: the kernel time of the last jpt_encode
 * in ms, when it ran under jpt_set_kernel_timing (else JPT_E_STATE); it waits for it.
 * Not covered: BC6H or any block compression, R11G11B10F, a jpt_multi_* form, the guide and bake-texel images, dithering. */
typedef enum { JPT_ENCODE_RGBA16F = 1, JPT_ENCODE_RGB9E5 = 2, JPT_ENCODE_RGBE8 = 3 } jpt_encode_format;
typedef enum { JPT_ENCODE_SOURCE_MEAN = 0, JPT_ENCODE_SOURCE_DENOISED = 1, JPT_ENCODE_SOURCE_DISPLAY = 2,
               JPT_ENCODE_SOURCE_LIGHTMAP = 3, JPT_ENCODE_SOURCE_REFLECTION = 4, JPT_ENCODE_SOURCE_PROBE_SH = 5 } jpt_encode_source;
#define JPT_ENCODE_ALL_LEVELS (-1)
typedef struct { int32_t source, format, level, width, height; uint64_t n_texels, bytes; } jpt_encoded_info;
int   jpt_encode(jpt_ctx *ctx, int32_t source, int32_t level, int32_t format);
int   jpt_get_encoded_info(jpt_ctx *ctx, jpt_encoded_info *out);
int   jpt_read_encoded(jpt_ctx *ctx, void *out, size_t capacity);
int   jpt_readback_encoded_begin(jpt_ctx *ctx);
int   jpt_readback_encoded_end(jpt_ctx *ctx, void *out, size_t capacity);
void *jpt_device_encoded(jpt_ctx *ctx, size_t *bytes_out);
int   jpt_get_encode_timing(jpt_ctx *ctx, float *ms);

/* ---- metering: a luminance histogram and auto-exposure on the device (no reference counterpart; Godot's
 * CameraAttributes.auto_exposure_*) -----------------------------------------------------------------------------------
 * jpt_meter builds a 256-bin log-luminance histogram of the running mean and resolves it, on the device, into one exposure value;
 * jpt_set_auto_exposure lets jpt_display multiply by that value straight from device memory.  The host never waits and never reads an
 * image; it may read the 1 KB histogram and the 32-byte result for a UI.  An explicit call: nothing runs unless the host asks, and
 * with the switch off, or with none of these calls made, every render, buffer, read-back and jpt_display image and
 * jpt_get_workspace_bytes are exactly what they are without this section.  The arithmetic is pinned in DESIGN.md section 2
 * (gdpathtracing_amd/csrc/jpt_meter.h; tests/np_meter.py restates it bit for bit):
 *   per pixel   m = accum.rgb / frame_count (JPT_DISPLAY_SOURCE_DENOISED: jpt_denoise's image); lum = 0.2126 m.r + 0.7152 m.g +
 *               0.0722 m.b; a pixel with a non-finite channel or without lum > 0 is skipped; bin = clamp((bits(lum) >> 20) - 856,
 *               0, 255): eight bins per octave, bin 0 from 2^-20, bin 255 to 2^12, darker and brighter values in the end bins;
 *               hist[bin] += 1, or 4 under JPT_METER_CENTER_WEIGHTED where 4x >= W, 4x < 3W, 4y >= H and 4y < 3H
 *   resolve     (uint64) total = sum of the bins; lo = total * low_permille / 1000; hi = total * high_permille / 1000; of each bin,
 *               in ascending order, the part c[b] of its weight between lo and hi; used = sum c[b]; S = sum c[b] (2b + 1).
 *               used == 0 (JPT_METER_EMPTY): the exposure stays (a FIRST call: clamp(1, min, max)).  Else p = S * 32768 / used,
 *               L_avg = the binary32 with the bits 0x35800000 + (p << 4), target = clamp(key / L_avg, min_exposure, max_exposure);
 *               a FIRST call takes the target, any other exposure = prev + (target - prev) * adapt.
 *
 * jpt_meter enqueues on the context's stream, ordered as jpt_display is: behind every render, jpt_denoise and jpt_display queued
 * before it and ahead of what follows.  It READS the accumulation and the frame count, or jpt_denoise's image, and writes only its
 * own buffers: the 256 uint32 bins, 16 working sets of them (17 KB in all) and a 32-byte state record, allocated at the first call,
 * freed by jpt_destroy; jpt_get_workspace_bytes does not count them.  The state is reset
 * (the next jpt_meter is a FIRST one) by jpt_set_params with another size and by jpt_meter_reset.  jpt_read_meter waits for the work
 * queued on the context and reads through its pinned staging buffer.
 * JPT_E_STATE: a denoising mode other than JPT_DENOISE_PROGRESSIVE; the DEBUG_STEPS mode; a screen partition; jpt_set_params not
 * called; no frame accumulated since the last reset; source = DENOISED without a jpt_denoise at the current resolution; an image
 * without pixels; jpt_read_meter without a jpt_meter since the state was reset.  JPT_E_LIMIT: width * height > 2^30 (a weight is at
 * most 4 and a bin is a uint32).  JPT_E_INVALID outside the ranges below or for a non-finite value.  Host-only contexts:
 * JPT_E_DEVICE, after the checks that need no device.  The parameters and the auto-exposure switch are the context's: they survive
 * scene changes, each call takes them by value, jpt_scene_share does not copy them; jpt_set_meter_params never resets the state.
 *
 * jpt_set_auto_exposure(ctx, 1): jpt_display uses params.exposure * state.exposure wherever it uses exposure (the bloom's base and
 * the resolve; one binary32 multiply per use), so that params.exposure becomes the exposure compensation.  state.exposure is read
 * on the device, as the last jpt_meter before the jpt_display on the stream left it.  JPT_E_STATE from jpt_display when no jpt_meter
 * ran since the state was reset.  There is no jpt_multi_* form and nothing under a partition, as for jpt_display. */
enum { JPT_METER_AVERAGE = 0, JPT_METER_CENTER_WEIGHTED = 1 };
enum { JPT_METER_EMPTY = 1, JPT_METER_FIRST = 2 };           /* jpt_meter_result.flags */
typedef struct jpt_meter_params {
    int32_t source;          /* JPT_DISPLAY_SOURCE_ACCUM (default) or _DENOISED */
    int32_t mode;            /* default JPT_METER_AVERAGE */
    int32_t low_permille;    /* 0..1000, default 100: this share of the weight, from the dark end, is ignored */
    int32_t high_permille;   /* low < high <= 1000, default 900 */
    float   key;             /* finite, > 0, default 0.18: the luminance the metered value is mapped to */
    float   min_exposure;    /* finite, > 0, default 1/64 */
    float   max_exposure;    /* finite, >= min, default 64 */
    float   adapt;           /* [0, 1], default 1: share of the way to the target taken per jpt_meter
                                (the host passes 1 - exp(-dt * speed)) */
} jpt_meter_params;
typedef struct jpt_meter_result {
    float exposure;          /* the state after the call */
    float target;            /* the target of this call (exposure when EMPTY) */
    float luminance;         /* L_avg (0 when EMPTY) */
    uint32_t flags;
    uint64_t weight;         /* total histogram weight */
    uint64_t used;           /* weight left after the clipping */
} jpt_meter_result;          /* 32 B */
int jpt_set_meter_params(jpt_ctx *ctx, const jpt_meter_params *params);   /* NULL: the defaults; never resets the state */
int jpt_meter(jpt_ctx *ctx);                                              /* enqueue; ordered as jpt_display is */
int jpt_meter_reset(jpt_ctx *ctx);                                        /* the next jpt_meter is a FIRST one */
int jpt_read_meter(jpt_ctx *ctx, jpt_meter_result *out, uint32_t *hist256 /* may be NULL */);
int jpt_set_auto_exposure(jpt_ctx *ctx, int32_t enable);                  /* default 0 */

/* ---- per-pixel noise: is the image finished? (no reference counterpart; the noise threshold of a production progressive renderer,
 * and the stop criterion of a LightmapGI-style bake: INTEGRATION.md) -------------------------------------------------------------------
 * With jpt_set_variance on, every render on the default kernel keeps one more float4 per pixel of the context's rows beside the
 * accumulation: (M2.r, M2.g, M2.b, 0), M2 = sum over the frames of (cur_f - mean)^2 per channel, cur_f the frame's value exactly as the
 * accumulation adds it (in JPT_ACCUM_REF_LDR8 the rgba8 value read back).  jpt_noise_estimate reduces the two planes, on the device,
 * to a histogram, a map of 8 x 8 tiles and one 32-byte answer; jpt_render_converge is the loop a caller would write around them.  The
 * host never reads a pixel.  The arithmetic is pinned in DESIGN.md section 2 (gdpathtracing_amd/csrc/jpt_variance.h;
 * tests/np_variance.py restates it bit for bit); every operation is one binary32 operation in the order written:
 *   per frame   k = the frame's count since the reset (1: the first); sum = the accumulation's own sum with this frame added
 *               (k == 1: cur; else cur + sum).  k == 1: m2 = +0, whatever the plane held.  k >= 2: kf = (float)k;
 *               d = kf * cur - sum;  w = 1.0f / (kf * (kf - 1.0f));  m2 = m2 + (d * d) * w.
 *               In real arithmetic this is Welford's update, (x - mean_old)(x - mean_new) = (k x - sum_k)^2 / (k (k - 1)); no term is
 *               negative, so m2 never is.  A pixel whose frames are all equal need not give exactly 0: k * x and x + x + ... round
 *               differently, and the result is of order x^2 * 2^-48.  The divisor is the caller's: M2 / (n - 1) is the sample variance
 *               of a frame, M2 / (n (n - 1)) the variance of the mean.
 *   per pixel   nf = (float)frame_count;  q = nf * (nf - 1.0f);  mean.c = sum.c / nf;  v.c = m2.c / q;
 *               lm = 0.2126f * mean.r + 0.7152f * mean.g + 0.0722f * mean.b;  lv = the same of v;  e = sqrt(lv) / (lm + floor): the
 *               relative standard error of the mean (lv is a noise measure, not the variance of the luminance: no covariance is kept).
 *               Counted: the six inputs finite, lm >= 0 and, in a bake render, a valid texel.  A counted pixel's bin is
 *               clamp((bits(e) >> 20) - 856, 0, 255): eight bins per octave from 2^-20, e = 0 in bin 0; it is "above" when
 *               e > threshold.  A pixel that is not counted contributes to nothing.
 *   outputs     hist[256], uint32, of the counted pixels; tiles[ceil(W / 8) * ceil(H / 8)], float, row-major: the largest e > 0 of
 *               the tile's counted pixels, or 0; the result: `error` = the upper edge, the binary32 with the bits (b + 1 + 856) << 20,
 *               of the first bin b at which the cumulative count reaches ceil(counted * percentile_permille / 1000); `max_error` = the
 *               maximum over the tile map; `tiles_above` = the tiles whose value is > threshold.  JPT_NOISE_EMPTY: frame_count < 2 or
 *               counted == 0; then error = max_error = 0 and the result is not converged.  JPT_NOISE_CONVERGED: not empty and
 *               above * 1000 <= counted * allowed_permille.  Sums are integers and maxima are of non-negative floats: nothing depends
 *               on the order the pixels arrive in.
 *
 * jpt_set_variance             a switch of the context, as jpt_set_bake_directional: it survives commits and uploads, jpt_scene_share
 *                              does not copy it, and a CHANGE of the value resets the accumulation as jpt_accum_reset does.  With the
 *                              switch on a render launches one kernel of its own in front of its accumulation (no path kernel
 *                              differs) and a pinhole render takes no sky cull, as a lens render: every pixel's frames are then kept
 *                              until the accumulation has read them.  The accumulation, display and depth images stay bit for bit
 *                              what they are with the switch off; with the switch off no launch, argument, allocation or output of
 *                              any render differs.  Works with every kind of primary ray, lighting family, both accumulation modes,
 *                              queued renders and a partition (each rank keeps its own rows).
 * jpt_read_variance_f32        W * H * 4 floats, scattered to image rows as jpt_read_accum_f32 does.  Waits for the renders queued so far.
 * jpt_device_variance          the plane's device pointer and size (the context's own rows, local order); NULL and 0 when there is none.
 * jpt_set_noise_params         NULL: the defaults.  JPT_E_INVALID outside the ranges below.
 * jpt_noise_estimate           enqueues on the context's stream, ordered as jpt_meter is; it READS the accumulation, the plane, the
 *                              frame count and (bake renders) the normal image and writes only its own buffers.
 * jpt_read_noise               waits, and reads the 32-byte result and, optionally, the 1 KB histogram.
 * jpt_read_noise_tiles_f32     the tile map; jpt_device_noise_tiles: its device pointer, for a later pass on the device.
 * jpt_render_converge          repeats jpt_render_async(frames_per_step) at consecutive frame indices from first_frame_index,
 *                              jpt_noise_estimate and jpt_read_noise until the result is converged or max_frames frames are done (the
 *                              last step is shortened to land on it): the host waits once per step, for 32 bytes.  *frames_done: the
 *                              frames rendered by the call; *last: the last result.  Either may be NULL.  The accumulation is not
 *                              reset: the frames add to those already there.
 * Memory (jpt_get_workspace_bytes is about the workspace and does not count these): 16 B per pixel of the context's rows for the
 * plane, made by the first render with the switch on, freed when it goes off; 4 B per 8 x 8 tile for the tile map; 17.3 KB of bins
 * (256 published, 16 working sets) and the 32-byte record, made by the first jpt_noise_estimate.
 * JPT_E_STATE, with a message naming jpt_set_variance: a render with the switch on under JPT_KERNEL_REFERENCE_LAYOUT (it adds frame
 * by frame and keeps no per-frame values), a denoising mode other than JPT_DENOISE_PROGRESSIVE, or jpt_set_debug_steps.
 * jpt_read_variance_f32 / jpt_device_variance with the switch off or before the first render with it on: JPT_E_STATE / NULL.
 * jpt_noise_estimate: jpt_meter's refusals (the mode, DEBUG_STEPS, a screen partition, jpt_set_params not called, no frame), the switch
 * off, no render with it on at the current size.  jpt_read_noise / jpt_read_noise_tiles_f32 before a jpt_noise_estimate at the current
 * size: JPT_E_STATE.  jpt_render_converge: an argument <= 0 is JPT_E_INVALID; otherwise the refusals of the calls it makes.
 * Host-only contexts: JPT_E_DEVICE.  There is no jpt_multi_* form.
 * Not covered: adaptive sampling (skipping converged tiles would edit the primary launch),
 * jpt_multi and an estimate under a partition, a jpt_encode source for the plane, the reference-layout kernel, per-channel covariance. */
enum { JPT_NOISE_EMPTY = 1, JPT_NOISE_CONVERGED = 2 };       /* jpt_noise_result.flags */
typedef struct jpt_noise_params {
    float   threshold;            /* default 0.05: a pixel, or a tile, is "above" when its e is greater */
    float   floor;                /* finite, > 0, default 0.01: added to the mean luminance, so that dark pixels do not rule */
    int32_t percentile_permille;  /* 1..1000, default 950: `error` is this percentile of e over the counted pixels */
    int32_t allowed_permille;     /* 0..1000, default 0: the share of counted pixels that may stay above the threshold */
} jpt_noise_params;
typedef struct jpt_noise_result {
    float error;             /* the percentile of e, as the upper edge of its bin (0 when EMPTY) */
    float max_error;         /* the largest e of any counted pixel (0 when EMPTY) */
    uint32_t flags;
    uint32_t tiles_above;    /* tiles whose largest e is > threshold */
    uint64_t counted;        /* pixels counted */
    uint64_t above;          /* ... of which e > threshold */
} jpt_noise_result;          /* 32 B */
int   jpt_set_variance(jpt_ctx *ctx, int32_t enable);                        /* default 0 */
int   jpt_read_variance_f32(jpt_ctx *ctx, float *out);                       /* W*H*4 floats: (M2.r, M2.g, M2.b, 0) */
void *jpt_device_variance(jpt_ctx *ctx, size_t *bytes_out);
int   jpt_set_noise_params(jpt_ctx *ctx, const jpt_noise_params *params);    /* NULL: the defaults */
int   jpt_noise_estimate(jpt_ctx *ctx);                                      /* enqueue; ordered as jpt_meter is */
int   jpt_read_noise(jpt_ctx *ctx, jpt_noise_result *out, uint32_t *hist256 /* may be NULL */);
int   jpt_read_noise_tiles_f32(jpt_ctx *ctx, float *out);                    /* ceil(W/8) * ceil(H/8) floats */
void *jpt_device_noise_tiles(jpt_ctx *ctx, size_t *bytes_out);
int   jpt_render_converge(jpt_ctx *ctx, int32_t frames_per_step, int32_t max_frames, uint32_t first_frame_index, int32_t *frames_done,
                          jpt_noise_result *last);

/* ---- ray queries: what does this ray hit? (no reference counterpart) ---------------------------------------------------------------
 * Caller-supplied rays against the scene the device holds, as an explicit call: nothing runs unless the host asks, queries change no
 * statistic of jpt_stats and no buffer a render or a read-back reads.  For picking, autofocus, line of sight and
 * probe rays against the scene the renderer shows, device-side refits and mesh updates included.
 *
 * The scene walked: the arrays the wavefront kernels walk, whatever jpt_set_kernel says -- the four-child records of a native tree,
 *   the two-child records of a JPT_BUILD_REFERENCE_EXACT or as-given tree -- with the copy of the instance level current at the call,
 *   chosen as jpt_denoise's guide pass chooses it: queries follow jpt_scene_refit_tlas, jpt_scene_update_tlas,
 *   jpt_scene_update_reference_tlas and jpt_scene_update_mesh (after which they WORK, unlike the host mirrors).
 * The hit rule: the guide pass's -- the smallest Moller-Trumbore t that intersectTriangle (main.glsl:224-257) accepts, no reach records
 *   and no tie walk.  At an exact distance tie ANY of the tying triangles may be returned.  On the reference's own trees a float crack
 *   between boxes can hide a triangle (the walk gives that tree's answer), as for the guides.  Glass blocks, as for shadow rays.
 * The ray: `dir` is used as given, not normalised; t is in units of its length, exactly as the kernels treat a ray.  The walk starts
 *   with hit.t = tmax, and a hit is a final hit.t < tmax.  A tmax that is NaN, <= 0 or >= 1e9 (infinity included) is taken as 1e9, the
 *   pipeline's miss sentinel.  A ray with a non-finite origin or direction component, or an all-zero direction, is not walked: its hit
 *   is the miss encoding with flags = JPT_HIT_BAD_RAY, its occlusion byte 0 (checked on the device: both forms behave alike).
 * JPT_QUERY_CLOSEST fills hits_out; occluded_out may be NULL, else one byte per ray: 1 on a hit, 0 otherwise.
 *   a miss: t = -1, instance = -1, flags = 0, everything else 0.
 *   a hit:  t, u, v as the walk found them; `instance` the instance whose local ray found the triangle; `triangle` in the device's
 *           triangle order = the order of JPT_BUF_TRI_GEOMETRY / JPT_BUF_TRI_DATA as jpt_scene_get_reference_buffer hands them out
 *           (after a native upload: the native order, not the caller's) and of jpt_debug_light_tables' pairs; `material` the index
 *           get_shading_data resolves (the instance's slot of the triangle's material_index; out of range: 0); flags =
 *           JPT_HIT_VALID | (JPT_HIT_FRONT when dot(cross(e1, e2), dir) > 0 in the instance's space); the world `position`, the
 *           facing shading `normal` and the interpolated `uv` of the shading record -- the call the guide pass makes, so position
 *           and normal of a pixel-centre ray equal jpt_read_guides_f32's texel bit for bit.
 * JPT_QUERY_ANY stops at the first accepted triangle with t < tmax and writes occluded_out only; hits_out must be NULL.
 * jpt_query_pixels: xy[2i], xy[2i + 1] are raster coordinates in pixels (x + 0.5, y + 0.5 is the centre of pixel (x, y)); the ray is
 *   cam.position and the un-jittered pinhole direction of the guide pass, mode CLOSEST, tmax 1e9.  It ignores jpt_set_lens, as the
 *   guide pass does, and follows jpt_set_camera_model, as the guide pass does: under PROJECTIVE or EQUIRECT the ray is the model's
 *   ray of the exact position, from its own origin.  Coordinates outside [0, width] x [0, height] are allowed (a ray is a ray); a non-finite one: JPT_HIT_BAD_RAY.
 * Ordering: all three enqueue on the context's stream, behind every render, refit, mesh update and jpt_denoise queued before them and
 *   ahead of what is queued after; jpt_scene_update_mesh's device-side wait covers the queries queued before it.  The host forms
 *   block: rays and results travel through the context's pinned staging buffer in chunks of at most 2^20 rays (n is unbounded, the
 *   memory is not: 97 B per ray of a chunk, pinned and on the device).  jpt_query_rays_device is asynchronous: the three pointers are
 *   device memory of the context's device, 16-byte aligned, n jpt_ray / n jpt_ray_hit / n bytes; jpt_sync, or work queued on
 *   jpt_get_stream's stream, orders against it.
 * n = 0 succeeds and touches nothing.  JPT_E_INVALID: an unknown mode, NULL where an array is required, hits_out with JPT_QUERY_ANY, a
 * misaligned or non-device pointer.  Host-only contexts: JPT_E_DEVICE, after those checks.  JPT_E_STATE: no scene; jpt_query_pixels
 * before jpt_set_params and jpt_set_camera. */
typedef struct jpt_ray {
    float origin[3]; float tmax;
    float dir[3];    uint32_t reserved;   /* not read */
} jpt_ray;                                /* 32 B */
typedef struct jpt_ray_hit {
    float t, u, v; int32_t instance;
    uint32_t triangle; int32_t material; uint32_t flags;
    float position[3]; float normal[3]; float uv[2];
    uint32_t reserved;                    /* written 0 */
} jpt_ray_hit;                            /* 64 B */
enum { JPT_HIT_VALID = 1, JPT_HIT_FRONT = 2, JPT_HIT_BAD_RAY = 4 };
enum { JPT_QUERY_CLOSEST = 0, JPT_QUERY_ANY = 1 };
int jpt_query_rays(jpt_ctx *ctx, int32_t mode, const jpt_ray *rays, uint32_t n, jpt_ray_hit *hits_out, uint8_t *occluded_out);
int jpt_query_rays_device(jpt_ctx *ctx, int32_t mode, const void *d_rays, uint32_t n, void *d_hits_out, void *d_occluded_out);
int jpt_query_pixels(jpt_ctx *ctx, const float *xy, uint32_t n, jpt_ray_hit *hits_out);

/* ---- outputs ---------------------------------------------------------------------------------- */

/* replaces: cs->get_image_uniform_buffer(output_texture_rid) (path_tracing_camera.cpp:228-229):
 * W*H*4 bytes, the screen image after ACES(sum / frame_count) (progressive_rendering.glsl:39-45).  Waits for the work
 * queued on the context; the bytes travel through the context's pinned staging buffer and one host copy, so `out` may be
 * ordinary (pageable) memory without the copy running at pageable speed. */
int jpt_read_ldr_rgba8(jpt_ctx *ctx, uint8_t *out);
/* Split form of jpt_read_ldr_rgba8 for double-buffered display (the reference stalls on
 * the read-back every frame, path_tracing_camera.cpp:228-230): `begin` enqueues the device->host copy of the
 * current screen image into a pinned staging buffer behind the work already queued on the context's stream
 * and returns at once; the host may queue the next jpt_render_async; `end` waits for that copy only and hands
 * the bytes out.  One read-back may be in flight per context. */
int jpt_readback_ldr_begin(jpt_ctx *ctx);
int jpt_readback_ldr_end(jpt_ctx *ctx, uint8_t *out);
/* the rgba32f frameBuffer (progressive_rendering.glsl:10,37): W*H*4 floats (like every jpt_read_*: through pinned staging) */
int jpt_read_accum_f32(jpt_ctx *ctx, float *out);
/* the r32f depthBuffer (main.glsl:99,435), last frame: W*H floats */
int jpt_read_depth_f32(jpt_ctx *ctx, float *out);

/* Device pointers of this context's LOCAL framebuffers (its partition's rows, strip-major), for
 * plumbing (RCCL gather through torch): float4 accumulation, and its size in bytes. */
void *jpt_device_accum(jpt_ctx *ctx, size_t *bytes_out);
/* Rank 0 after the gather: scatter `world` rank-major local buffers (device pointer) into this context's
 * full W*H framebuffers so jpt_read_* return the assembled image.  The gathering context's OWN rows are read in place,
 * from its local buffers as its last render left them: its slot of `device_gathered` is not read and need not be filled
 * (no copy of a rank's piece to itself). */
int jpt_assemble_from_ranks(jpt_ctx *ctx, const void *device_gathered, int32_t world);
/* The display image alone.  Every rank holds the complete sums of its own rows, so its rgba8 rows are final:
 * gathering them (4 bytes per pixel instead of 16) is all a displayed frame needs -- what the reference reads back
 * is this image (path_tracing_camera.cpp:228-229).  Afterwards jpt_read_ldr_rgba8 / jpt_readback_ldr_* on the
 * gathering rank return the whole image; the accumulation buffers stay distributed. */
void *jpt_device_ldr(jpt_ctx *ctx, size_t *bytes_out);
int jpt_assemble_ldr_from_ranks(jpt_ctx *ctx, const void *device_gathered_rgba8, int32_t world);
int32_t jpt_local_rows(jpt_ctx *ctx);

int jpt_get_stats(jpt_ctx *ctx, jpt_stats *out);

/* ---- one image on several GPUs from ONE process ------------------------------------------------------
 * The addon's host is a single C++ process (path_tracing_camera.cpp:193-232).  A jpt_multi owns one context per listed
 * device, each rendering its strips of the screen partition (jpt_set_partition); jpt_multi_render fans the render out,
 * every peer pushes its float4 accumulation rows to device 0 with a peer-to-peer copy over its own xGMI link (on a copy
 * stream of its own device, behind an event on the rank's render: the N - 1 transfers are in flight together, and the next
 * renders' path kernels overlap with them) and device 0 assembles them -- its own rows in place --, so the
 * jpt_multi_read_* calls return the whole image -- bit-identical to one GPU's.  Scene set-up: build it once on
 * jpt_multi_ctx(m, 0) with the jpt_scene_* calls, then jpt_multi_share_scene.  (Processes that hold one GPU each --
 * bench.py under torch.distributed -- use jpt_set_partition / jpt_device_accum / jpt_assemble_from_ranks with RCCL
 * send/recv in between instead.)  A device id may be listed more than once (rehearsal on a box with fewer GPUs). */
typedef struct jpt_multi jpt_multi;
int jpt_multi_create(const int *device_ids, int n_devices, jpt_multi **out);
void jpt_multi_destroy(jpt_multi *m);
const char *jpt_multi_last_error(const jpt_multi *m);     /* m may be NULL: error of the last failed jpt_multi_create */
int jpt_multi_world(const jpt_multi *m);
jpt_ctx *jpt_multi_ctx(jpt_multi *m, int rank);            /* the context of one rank (scene calls, statistics) */
int jpt_multi_share_scene(jpt_multi *m);                   /* jpt_scene_share(rank r, rank 0) for every other rank */
/* Moving instances under a jpt_multi: the moving-instance calls above, applied to EVERY rank's replica (a scene call made
 * on jpt_multi_ctx(m, 0) alone would leave the other ranks rendering their strips of the old scene state).  Same
 * arguments and results as jpt_scene_set_instance_transform / jpt_scene_update_tlas / jpt_scene_refit_tlas /
 * jpt_scene_update_reference_tlas; the first failing rank's error is reported. */
int jpt_multi_set_instance_transform(jpt_multi *m, uint32_t instance, const float *transform12);
int jpt_multi_update_tlas(jpt_multi *m);
int jpt_multi_refit_tlas(jpt_multi *m, const float *transforms12, uint32_t n_instances);
int jpt_multi_rebuild_tlas(jpt_multi *m, const float *transforms12, uint32_t n_instances);
int jpt_multi_update_reference_tlas(jpt_multi *m, const void *blas_instances, uint32_t n_instances,
                                    const void *tlas_nodes, uint32_t n_tlas_nodes);
/* jpt_scene_update_mesh on every rank's replica */
int jpt_multi_update_mesh(jpt_multi *m, uint32_t mesh_id, const jpt_surface *surfaces, int32_t n_surfaces);
/* jpt_scene_set_mesh_rig / jpt_scene_pose_mesh / jpt_scene_clear_mesh_rig on every rank's replica */
int jpt_multi_set_mesh_rig(jpt_multi *m, uint32_t mesh_id, const jpt_surface *bind, const jpt_surface_rig *rigs,
                           int32_t n_surfaces, int32_t influences, int32_t n_blend_shapes);
int jpt_multi_pose_mesh(jpt_multi *m, uint32_t mesh_id, const float *bone_transforms12, uint32_t n_bones,
                        const float *blend_weights, uint32_t n_blend_weights);
int jpt_multi_clear_mesh_rig(jpt_multi *m, uint32_t mesh_id);
/* jpt_scene_rebuild_mesh / jpt_scene_pose_mesh_rebuild on every rank's replica */
int jpt_multi_rebuild_mesh(jpt_multi *m, uint32_t mesh_id, const jpt_surface *surfaces, int32_t n_surfaces);
int jpt_multi_pose_mesh_rebuild(jpt_multi *m, uint32_t mesh_id, const float *bone_transforms12, uint32_t n_bones,
                                const float *blend_weights, uint32_t n_blend_weights);
int jpt_multi_set_params(jpt_multi *m, int32_t width, int32_t height, int32_t max_bounces, int32_t accum_mode, int32_t sampler_mode);
/* jpt_set_environment / jpt_set_environment_params on every rank */
int jpt_multi_set_environment(jpt_multi *m, const float *rgb, int32_t width, int32_t height);
int jpt_multi_set_environment_params(jpt_multi *m, const float *rotation9, float intensity);
int jpt_multi_set_environment_sampling(jpt_multi *m, int32_t mode);
/* jpt_set_sky on every rank */
int jpt_multi_set_sky(jpt_multi *m, const jpt_sky_params *params, int32_t width, int32_t height, int32_t samples);
int jpt_multi_set_light_sampling(jpt_multi *m, int32_t mode);
int jpt_multi_set_material_extensions(jpt_multi *m, uint32_t flags);
/* jpt_set_lens on every rank */
int jpt_multi_set_lens(jpt_multi *m, float aperture_radius, float focus_distance);
/* jpt_set_camera_model on every rank */
int jpt_multi_set_camera_model(jpt_multi *m, int32_t model);
/* jpt_set_bake_texels on every rank (each holds the whole images) */
int jpt_multi_set_bake_texels(jpt_multi *m, const float *position4, const float *normal4, int32_t width, int32_t height);
int jpt_multi_set_camera(jpt_multi *m, const void *camera160);
int jpt_multi_accum_reset(jpt_multi *m);
/* what crosses the links each render: 0 (default) the float4 accumulation rows (16 B per pixel; BASELINE.json's exchange),
 * 1 only the finished rgba8 display rows (4 B per pixel, what the reference reads back) */
int jpt_multi_set_gather(jpt_multi *m, int32_t ldr_only);
/* asynchronous: queues the render on every rank, the gather and the assembly; jpt_multi_sync or a read waits */
int jpt_multi_render(jpt_multi *m, int32_t n_frames, uint32_t first_frame_index);
int jpt_multi_sync(jpt_multi *m);
/* What the last jpt_multi_render issued for its gather (diagnostic; SURVEY.md 8(e): the N - 1 transfers must be concurrent,
 * one per xGMI link): the number of peer copies, the number of DISTINCT streams they were issued on (each peer pushes on a
 * stream of its own device: = n_peer_copies), and how often rank 0's own piece was copied (0: the assembly reads it in place). */
int jpt_multi_gather_plan(const jpt_multi *m, int32_t *n_peer_copies, int32_t *n_distinct_streams, int32_t *own_piece_copies);
int jpt_multi_read_ldr_rgba8(jpt_multi *m, uint8_t *out);
int jpt_multi_read_accum_f32(jpt_multi *m, float *out);

/* ---- audit entry points (tests; no reference counterpart) ---------------------------------------------------------------
 * The native walk's box tests are conservative tests on quantised planes.  These run that one step
 * on caller-made inputs so its conservativeness can be tested directly (tests/test_quantized_walk.py), not only sampled
 * through images. */
/* n_nodes four-child records in the float form (128 bytes each: lo_x[4] lo_y[4] lo_z[4] child[4] hi_x[4] hi_y[4] hi_z[4]
 * pad[4]; an unused slot has child = INT32_MIN) -> their 64-byte quantised form, with the function uploads use. */
int jpt_debug_quantize_nodes4(const void *nodes4, uint32_t n_nodes, void *nodesq_out);
/* One record step per case.  A case is 32 bytes: ray origin xyz, direction xyz (as the walk holds them: the local ray of the
 * level), the closest distance found so far (hitInfo.t), and the index of the record to expand.  The records' child
 * references must be k + 1 for slot k.  taken_out[i] gets bit k set when the walk keeps child k (descends into it or
 * pushes it).  device_id >= 0: the kernel runs the very function the tracing kernels inline.  JPT_DEVICE_HOST_ONLY: a
 * host restatement of the same arithmetic, with its reciprocals moved host_rcp_ulps ulps away from zero (negative: towards
 * zero) -- v_rcp_f32 is accurate to 1 ulp. */
int jpt_debug_node_step4(int device_id, const void *nodes4, uint32_t n_nodes, const void *cases32, uint32_t n_cases,
                         int32_t host_rcp_ulps, uint8_t *taken_out);
const char *jpt_debug_last_error(void);
/* The environment lookup (jpt_set_environment) for n directions: rgb_out[3 i .. 3 i + 2] = env_radiance of dirs3[3 i .. 3 i + 2]
 * with the map (rgb, width, height), rotation9 (NULL: identity) and intensity, checked as jpt_set_environment /
 * jpt_set_environment_params check them.  device_id >= 0: the function the kernels inline, on that device;
 * JPT_DEVICE_HOST_ONLY: the same function compiled for the host. */
int jpt_debug_env_lookup(int device_id, const float *rgb, int32_t width, int32_t height, const float *rotation9,
                         float intensity, const float *dirs3, uint32_t n, float *rgb_out);
/* The map sampler of JPT_ENV_SAMPLING_MIS for the map (rgb, width, height) and rotation9 (NULL: identity; checked as
 * jpt_set_environment_params checks it with MIS on), device_id >= 0 on that device (tables built by the kernels the context
 * uses), JPT_DEVICE_HOST_ONLY the same functions compiled for the host:
 *   _tables: cond_out[height * width] the per-row conditional CDFs, marg_out[height] the marginal CDF, total_out[0] the total
 *            weight (any output may be NULL);
 *   _sample: for xi2[2 i], xi2[2 i + 1] (column and row randoms in [0, 1]): dirs_out[3 i ..] the world direction and pdf_out[i]
 *            its density per steradian (0 and a zero direction for a black map);
 *   _pdf:    pdf_out[i] = the density of world direction dirs3[3 i ..]. */
int jpt_debug_env_tables(int device_id, const float *rgb, int32_t width, int32_t height, float *cond_out, float *marg_out,
                         float *total_out);
int jpt_debug_env_sample(int device_id, const float *rgb, int32_t width, int32_t height, const float *rotation9,
                         const float *xi2, uint32_t n, float *dirs_out, float *pdf_out);
int jpt_debug_env_pdf(int device_id, const float *rgb, int32_t width, int32_t height, const float *rotation9,
                      const float *dirs3, uint32_t n, float *pdf_out);
/* The procedural sky of jpt_set_sky, checked as that call checks its arguments (params NULL: the defaults):
 *   _sky:          rgb_out[3 (j width + i) ..] = texel (i, j) of the width x height map; device_id >= 0 launches the kernel on that
 *                  device, JPT_DEVICE_HOST_ONLY runs the same functions in a host loop;
 *   _sky_radiance: rgb_out[3 i ..] = sky_radiance of the unit direction dirs3[3 i ..], one sample, on the host;
 *   _pow01:        out[i] = pow01_(b[i], e[i]), the pinned b^e for b in [0, 1] and e in [1/8, 64], on the host. */
int jpt_debug_sky(int device_id, const jpt_sky_params *params, int32_t width, int32_t height, int32_t samples, float *rgb_out);
int jpt_debug_sky_radiance(const jpt_sky_params *params, const float *dirs3, uint32_t n, float *rgb_out);  /* host; theta = atan2_(|d.xz|, d.y) */
int jpt_debug_pow01(const float *b, const float *e, uint32_t n, float *out);                              /* host */
/* The emitter tables of JPT_LIGHT_SAMPLING_MIS as the context's next render would take them (made now if stale; the context needs
 * a scene): n_out[0] = emitters, n_out[1] = blocks; then, each output may be NULL and is filled only if its capacity (in emitters)
 * is at least the count:
 *   _tables: pairs_out[2 i ..] (instance, triangle), tri_out[12 i ..] P0.xyz Le.r E1.xyz Le.g E2.xyz Le.b, cdf_out[i], and
 *            marg_out[0 .. blocks] (the marginal CDF, then the total);
 *   _sample: for xi4[4 i .. 4 i + 3] and origins3[3 i ..] (o, as the estimator's): points_out[3 i ..] = y, dirs_out[3 i ..] = l,
 *            pdf_out[i] = p_L (0 when c = 0 or the total is 0);
 *   _pdf:    pdf_out[i] = p_L of hit point points3[3 i ..] on triangle tri[i] of instance inst[i] seen from origins3[3 i ..]
 *            along dirs3[3 i ..] (the weight's density; 0 when lum(Le) = 0).
 * Host-only contexts: JPT_E_DEVICE. */
int jpt_debug_light_tables(jpt_ctx *ctx, uint32_t capacity, uint32_t *n_out, uint32_t *pairs_out, float *tri_out, float *cdf_out,
                           float *marg_out);
int jpt_debug_light_sample(jpt_ctx *ctx, const float *xi4, const float *origins3, uint32_t n, float *points_out, float *dirs_out,
                           float *pdf_out);
int jpt_debug_light_pdf(jpt_ctx *ctx, const uint32_t *inst, const uint32_t *tri, const float *points3, const float *origins3,
                        const float *dirs3, uint32_t n, float *pdf_out);
/* The dielectric event of JPT_MATERIAL_EXT_TRANSMISSION for n cases: facing normal normals3[3 i ..], out direction out_dirs3[3 i ..],
 * ior[i] (sanitised as the materials' is), front[i] != 0 for a front face and the lobe random xi_f[i]: dirs_out[3 i ..] = the next
 * direction, fresnel_out[i] = F (1 under total internal reflection), event_out[i] = 0 refract, 1 reflect, 2 total internal
 * reflection.  device_id >= 0: the function the kernels inline, on that device; JPT_DEVICE_HOST_ONLY: the same function compiled
 * for the host. */
int jpt_debug_dielectric(int device_id, const float *normals3, const float *out_dirs3, const float *ior, const uint8_t *front,
                         const float *xi_f, uint32_t n, float *dirs_out, float *fresnel_out, uint8_t *event_out);
/* The ray generation of a render with jpt_set_lens(aperture_radius, focus_distance) (radius 0: the pinhole's) for every pixel of
 * one frame of a width x height image seen through camera160: origins3_out / dirs3_out[3 (y width + x) ..] = the origin and the
 * direction of the path of pixel (x, y) and frame frame_index.  Lens arguments are checked as jpt_set_lens checks them; a basis
 * that is not finite: JPT_E_STATE.  device_id >= 0: the functions the kernels inline, on that device; JPT_DEVICE_HOST_ONLY: the same
 * functions compiled for the host. */
int jpt_debug_lens_rays(int device_id, const void *camera160, int32_t width, int32_t height, uint32_t frame_index,
                        float aperture_radius, float focus_distance, float *origins3_out, float *dirs3_out);
/* The ray generation of a render under jpt_set_camera_model(model) (PINHOLE: primary_ray's) for every pixel of one frame of a width
 * x height image seen through camera160, laid out as jpt_debug_lens_rays lays its rays out.  The model is checked as
 * jpt_set_camera_model checks it; EQUIRECT with a basis, or PROJECTIVE with an ivp, that is not finite: JPT_E_STATE.  device_id >= 0:
 * the functions the kernels inline, on that device; JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_camera_rays(int device_id, const void *camera160, int32_t width, int32_t height, uint32_t frame_index, int32_t model,
                          float *origins3_out, float *dirs3_out);
/* The first rays of a bake render's paths (jpt_set_bake_texels) for every texel of frame frame_index of width x height images:
 * origins3_out / dirs3_out [3 (y * width + x) ..] and valid_out[y * width + x] = 1, or zeros and 0 for an invalid texel.  The size is
 * checked as jpt_set_bake_texels checks it; the texels are taken as they are.  device_id >= 0: the function the kernels inline, on that
 * device; JPT_DEVICE_HOST_ONLY: the same function compiled for the host. */
int jpt_debug_bake_rays(int device_id, const float *position4, const float *normal4, int32_t width, int32_t height,
                        uint32_t frame_index, float *origins3_out, float *dirs3_out, uint8_t *valid_out);
/* jpt_bake_add_surface on all-invalid width x height images, which it returns: the arguments are checked as that call checks them.
 * device_id >= 0: the kernels the context runs, on that device; JPT_DEVICE_HOST_ONLY: a plain loop over texels and triangles calling
 * the same coverage and resolve functions compiled for the host. */
int jpt_debug_bake_raster(int device_id, const jpt_surface *surface, const float *uv2, const float *transform12,
                          int32_t width, int32_t height, float *position4_out, float *normal4_out);
/* The whole transform of jpt_bake_finish on caller-made images of width x height texels, 4 floats per texel each: mean4 = (mean r, g,
 * b, unused) is taken as the mean itself (frame count 1), position4 / normal4 as jpt_set_bake_texels takes them, out = the lightmap
 * (r, g, b, coverage).  params NULL: the defaults.  The arguments are checked as the context calls check theirs (the parameters, the
 * size -- more than 2^26 texels: JPT_E_LIMIT --, a valid texel with a non-finite position or normal).  device_id >= 0: the kernels
 * jpt_bake_finish launches, on that device; JPT_DEVICE_HOST_ONLY: the same functions compiled for the host, in plain loops. */
int jpt_debug_bake_finish(int device_id, int32_t width, int32_t height, const jpt_bake_finish_params *params,
                          const float *mean4, const float *position4, const float *normal4, float *out);
/* The moments of jpt_set_bake_directional on the host: the functions the moment kernel inlines (jpt_bake_dir.h), compiled for the host,
 * in a plain loop over the texels of width x height images and the n_frames frames of radiance3 [3 ((f * height + y) * width + x) ..],
 * frame f being frame first_frame_index + f.  accum_mode: JPT_ACCUM_HDR_F32 takes a frame's value as it is, JPT_ACCUM_REF_LDR8 through
 * the rgba8 store and load.  frame_count >= 1 is that of the first frame: 1 overwrites moments_inout, more continues the sums it holds.
 * moments_inout: 3 * width * height * 4 floats, laid out as jpt_read_bake_directional_f32's.  The size and the images are checked as
 * jpt_set_bake_texels checks them. */
int jpt_debug_bake_moments(const float *position4, const float *normal4, int32_t width, int32_t height, const float *radiance3,
                           int32_t n_frames, uint32_t first_frame_index, uint32_t frame_count, int32_t accum_mode, float *moments_inout);
/* The first rays of a probe render's paths (jpt_set_probes) for every pixel of frame frame_index of the image the probes make (width
 * = probes_per_row * tile_w, height = ceil(n_probes / probes_per_row) * tile_h): origins3_out / dirs3_out [3 (y * width + x) ..] and
 * valid_out[y * width + x] = 1, or zeros and 0 for a pixel of a tile without a probe.  The arguments are checked as jpt_set_probes
 * checks them.  device_id >= 0: the function the kernels inline, on that device; JPT_DEVICE_HOST_ONLY: the same, compiled for the host. */
int jpt_debug_probe_rays(int device_id, const float *position3, int32_t n_probes, int32_t tile_w, int32_t tile_h,
                         int32_t probes_per_row, uint32_t frame_index, float *origins3_out, float *dirs3_out, uint8_t *valid_out);
/* The quadrature table jpt_probe_project makes on the host for (tile_w, tile_h, flags): tile_w * tile_h * 9 floats, cell-major
 * (c = j * tile_w + i), the nine coefficients of a cell together. */
int jpt_debug_probe_basis(int32_t tile_w, int32_t tile_h, int32_t flags, float *table_out);
/* The projection of jpt_probe_project over a caller-made accumulation image (4 floats per pixel, the size the probes make), frame
 * count (>= 1) and table: sh_out = n_probes * 9 * 4 floats.  device_id >= 0: the kernel jpt_probe_project launches, on that device;
 * JPT_DEVICE_HOST_ONLY: the same sum in plain loops on the host. */
int jpt_debug_probe_project(int device_id, const float *accum4, uint32_t frame_count, int32_t n_probes, int32_t tile_w, int32_t tile_h,
                            int32_t probes_per_row, const float *table, float *sh_out);
/* The first rays of a cube render's paths (jpt_set_reflection_probes) for every pixel of frame frame_index of the image the probes make
 * (width = probes_per_row * 6 * face_size, height = ceil(n_probes / probes_per_row) * face_size): rays_out[6 (y * width + x) ..] = the
 * origin, then the direction; six zeros for a pixel of a strip without a probe.  The arguments are checked as
 * jpt_set_reflection_probes checks them.  device_id >= 0: the function the kernels inline, on that device; JPT_DEVICE_HOST_ONLY: the
 * same, compiled for the host. */
int jpt_debug_cube_rays(int device_id, const float *position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row,
                        uint32_t frame_index, float *rays_out);
/* The sample table jpt_reflection_prefilter makes on the host for output level `level` (1 .. n_levels - 1; n_levels 0: log2(face_size)
 * + 1) of (face_size, n_levels, samples): table_out = samples * 4 floats (L_x, L_y, L_z, w), src_level_out = samples bytes.  The kept
 * samples stand first, k ascending; the entries behind them are zeros with level byte 0xff, so the bytes say how many are kept. */
int jpt_debug_reflection_samples(int32_t face_size, int32_t n_levels, int32_t samples, int32_t level, float *table_out, uint8_t *src_level_out);
/* jpt_reflection_prefilter over a caller-made accumulation image (4 floats per pixel, the size the probes make) and frame count
 * (>= 1): out = level `level` of the chain, n_probes * 6 * s^2 float4.  params NULL: the defaults.  device_id >= 0: the kernels
 * jpt_reflection_prefilter launches, on that device; JPT_DEVICE_HOST_ONLY: the same functions in plain loops on the host. */
int jpt_debug_reflection_prefilter(int device_id, const float *accum4, uint32_t frame_count, int32_t n_probes, int32_t face_size,
                                   int32_t probes_per_row, const jpt_reflection_params *params, int32_t level, float *out);
/* The lens step alone, on the host, from caller-made randoms: for pinhole ray (origins3[3 i ..], dirs3[3 i ..]) and (xi2[2 i], xi2[2
 * i + 1]) the ray the lens of camera160 sends out (origins3_out, dirs3_out; either input ray kept when it does not point forward).
 * basis9_out (may be NULL): f, r, u.  The radius and the focus are taken as they are; a basis that is not finite is still returned,
 * with JPT_E_STATE. */
int jpt_debug_lens_sample(const void *camera160, float aperture_radius, float focus_distance, const float *origins3,
                          const float *dirs3, const float *xi2, uint32_t n, float *origins3_out, float *dirs3_out, float *basis9_out);
/* The filter of jpt_denoise alone, on caller-made images of width x height pixels, 4 floats per pixel each: mean4 = (mean r, g, b,
 * unused), the three guide images as jpt_read_guides_f32 lays them out, out = the denoised image (r, g, b, 1).  params NULL: the
 * defaults; checked as jpt_set_denoise_params checks them (JPT_E_INVALID; this call leaves no message).  device_id >= 0: the
 * kernels jpt_denoise launches, on that device; JPT_DEVICE_HOST_ONLY: the same weight function compiled for the host. */
int jpt_debug_atrous(int device_id, int32_t width, int32_t height, const jpt_denoise_params *params, const float *mean4,
                     const float *position_t, const float *normal, const float *albedo, float *out);
/* jpt_display's transform alone, on a caller-made image of width x height pixels, 4 floats per pixel: mean4 = (r, g, b, unused) is
 * taken as the image itself (frame count 1; params->source is checked and otherwise ignored).  out_f32 = the tone-mapped image (r,
 * g, b, 1), out_rgba8 = the encoded image; either may be NULL, not both.  params NULL: the defaults; checked as
 * jpt_set_display_params checks them (JPT_E_INVALID; this call leaves no message).  device_id >= 0: the kernels jpt_display
 * launches, on that device; JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_display(int device_id, int32_t width, int32_t height, const jpt_display_params *params, const float *mean4,
                      float *out_f32, uint8_t *out_rgba8);
/* The 255 code boundaries of JPT_TRANSFER_SRGB: out255[k - 1] = T[k], k = 1..255, the binary32 nearest to the sRGB decoding of
 * (k - 0.5) / 255; a value v is stored as the number of entries <= v. */
int jpt_debug_display_srgb_table(float *out255);
/* jpt_meter's pass alone, on a caller-made image of width x height pixels, 4 floats per pixel: mean4 = (r, g, b, unused) is taken as
 * the image itself (frame count 1; params->source is checked and otherwise ignored).  prev_exposure: the state before the call, or a
 * NaN for a FIRST call (an infinity: JPT_E_INVALID).  hist256_out (may be NULL): the 256 bins; result_out: the state after the
 * call.  params NULL: the defaults; checked as jpt_set_meter_params checks them (JPT_E_INVALID; this call leaves no message);
 * JPT_E_LIMIT for width * height > 2^30, reported after those refusals, so only for otherwise valid arguments.  device_id >= 0:
 * the kernels jpt_meter launches, on that device; JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_meter(int device_id, int32_t width, int32_t height, const jpt_meter_params *params, const float *mean4,
                    float prev_exposure, uint32_t *hist256_out, jpt_meter_result *result_out);
/* The update of jpt_set_variance on the host: the function the moment kernel inlines (jpt_variance.h), compiled for the host, in a
 * plain loop over the pixels of a width x height image and the n_frames frames of radiance3 [3 ((f * height + y) * width + x) ..].
 * accum_mode: JPT_ACCUM_HDR_F32 takes a frame's value as it is, JPT_ACCUM_REF_LDR8 through the rgba8 store and load.  frame_count >= 1
 * is that of the first frame: 1 overwrites sum_inout and m2_inout (whatever they held), more continues them.  Both are width *
 * height * 4 floats: (sum.r, sum.g, sum.b, 1) as the accumulation holds it, and (M2.r, M2.g, M2.b, 0). */
int jpt_debug_variance_moments(const float *radiance3, int32_t n_frames, uint32_t frame_count, int32_t accum_mode, float *sum_inout,
                               float *m2_inout, int32_t width, int32_t height);
/* jpt_noise_estimate's pass alone, on caller-made planes of width x height pixels, 4 floats per pixel: sum4 the accumulation, m2_4 the
 * plane, frame_count >= 1 the frames in them.  valid_or_null: one byte per pixel, 0 = a texel without a surface (a bake render), or
 * NULL for none.  hist256_out and tiles_out (ceil(width / 8) * ceil(height / 8) floats) may be NULL.  device >= 0: the kernels
 * jpt_noise_estimate launches, on that device; JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_noise_estimate(int device_id, int32_t width, int32_t height, const jpt_noise_params *params, const float *sum4,
                             const float *m2_4, uint32_t frame_count, const uint8_t *valid_or_null, uint32_t *hist256_out,
                             float *tiles_out, jpt_noise_result *result_out);
/* The filter of jpt_denoise with jpt_set_denoise_variance on, alone, on caller-made images of width x height pixels, 4 floats per
 * pixel each: sum4 the accumulation and m2_4 the plane of jpt_set_variance of frame_count >= 2 frames, the three guide images, out4 =
 * the denoised image (r, g, b, 1); var_out = width * height floats, v of the last pass.  params and vparams NULL: the defaults;
 * checked as their setters check them; vparams->enable is checked and otherwise ignored (JPT_E_INVALID, also for frame_count < 2;
 * this call leaves no message).  device_id >= 0: the kernels the guided jpt_denoise launches, on that device;
 * JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_atrous_variance(int device_id, int32_t width, int32_t height, const jpt_denoise_params *params,
                              const jpt_denoise_variance_params *vparams, const float *sum4, const float *m2_4, uint32_t frame_count,
                              const float *position_t, const float *normal, const float *albedo, float *out4, float *var_out);
/* The history stage of jpt_denoise alone (jpt_set_denoise_history), on caller-made planes of width x height pixels, 4 floats per
 * pixel each: sum4 the accumulation of frame_count >= 1 frames and the three guide images of this call; the previous history set as
 * three planes -- prev_integrated4 = (m.rgb, N), prev_normal_s4 = (normal, S), prev_position_t -- or three NULLs for none;
 * prev_vp16 the previous call's RefCamera vp, column-major (not read with same_view = 1 or without a previous set).  Outputs:
 * iv_out4 = (m.rgb, v_0), what the filter reads; integrated_out4 and normal_s_out4, the new set's first two planes (its third is
 * position_t).  params (normal_power_log2 is read) and hparams NULL: the defaults; checked as their setters check them; hparams->enable
 * is checked and otherwise ignored (JPT_E_INVALID; this call leaves no message).  device_id >= 0: history_kernel, on that device;
 * JPT_DEVICE_HOST_ONLY: the same functions compiled for the host. */
int jpt_debug_denoise_history(int device_id, int32_t width, int32_t height, const jpt_denoise_params *params,
                              const jpt_denoise_history_params *hparams, const float *sum4, uint32_t frame_count, const float *position_t,
                              const float *normal, const float *albedo, const float *prev_vp16, int32_t same_view,
                              const float *prev_integrated4, const float *prev_normal_s4, const float *prev_position_t, float *iv_out4,
                              float *integrated_out4, float *normal_s_out4);
/* The device's records of mesh `mesh_id` of a JPT_BUILD_SAH_WATERTIGHT commit, as stored (tests of jpt_scene_update_mesh):
 * info_out[6] = {1 if the device holds a tree for the mesh (an instance names it) else 0, its root reference, first record,
 * record count, first triangle, triangle count}.  Records: the float four-child records (128 B) and their quantised form
 * (64 B) of indices first .. first + count - 1 of the one index space (child references count from its start; a leaf
 * reference names triangles of the scene); triangles: WideTri (48 B: v0, nx, e1, ny, e2, nz) and ShadeTri (64 B: n0 n1 n2,
 * uvs, material slot) of the mesh's triangles in device order.  Any output may be NULL; capacities in records / triangles.
 * Waits for the context's stream. */
int jpt_debug_mesh_records(jpt_ctx *ctx, uint32_t mesh_id, void *nodes4_out, void *nodesq_out, uint32_t node_capacity,
                           void *tris_out, void *shade_out, uint32_t tri_capacity, int32_t *info_out);
/* jpt_scene_rebuild_tlas's steps alone (its tests).
 * jpt_debug_tlas_order: n <= 32 767 world boxes (lo3 / hi3: 3 floats per instance) -> the 45-bit key of every instance (keys_out, may
 *   be NULL: Morton code << 15 | index) and the instance at every position of the ascending order.  Per axis: c = (lo + hi) * 0.5f;
 *   bmin / bmax the least and greatest FINITE c; inv = bmax - bmin > 0 ? 1024.0f / (bmax - bmin) : 0; f = floor((c - bmin) * inv);
 *   cell = f >= 1024 ? 1023 : f >= 0 ? (uint32) f : 0, and 0 for a non-finite c; every step one binary32 operation.  device_id >= 0:
 *   the kernel the rebuild launches, on that device; device_id < 0: the same functions compiled for the host, sorted by std::sort.
 * jpt_debug_tlas_template: the tree over n sorted positions (2 <= n <= 32 767), 4 child words per record: >= 0 a record, ~position
 *   a leaf, or 0x80000000 an empty slot.  Records are numbered breadth first, record 0 the root over [0, n); a record over m <= 4
 *   positions holds them as its first slots; a record over more cuts its range into four parts of floor(m / 4), one more for the first
 *   m mod 4, a part of one position being a leaf slot.  n_records, n_levels, stack_need (the pending entries a walk of it can need):
 *   any may be NULL; child_out may be NULL, capacity in records.
 * jpt_debug_tlas_records: the TLAS records of the copy of the instance level new renders read, float (128 B) and quantised (64 B),
 *   internal child references counted from the first of them (root_out: the root's, 0 after a rebuild; negative: the root is an
 *   instance), and the world boxes of that copy's instance records (3 floats per instance each).  Any output may be NULL; capacity
 *   in records.  Waits for the context's stream. */
int jpt_debug_tlas_order(int device_id, const float *lo3, const float *hi3, uint32_t n, uint64_t *keys_out, uint32_t *sorted_instances_out);
int jpt_debug_tlas_template(uint32_t n, int32_t *child_out, uint32_t capacity, uint32_t *n_records, uint32_t *n_levels, uint32_t *stack_need);
int jpt_debug_tlas_records(jpt_ctx *ctx, void *nodes4_out, void *nodesq_out, uint32_t capacity, uint32_t *n_records, int32_t *root_out,
                           float *inst_lo3, float *inst_hi3);
/* jpt_scene_rebuild_mesh's order alone (its tests): n_tris triangles of three indices each into n_vertices vertices (3 floats each) ->
 * the 30-bit code of every triangle (codes_out, may be NULL) and the triangle (0 .. n_tris - 1) at every position of the order
 * ascending by (code, triangle), as jpt_scene_rebuild_mesh words it.  JPT_E_INVALID: a NULL array (n_tris > 0), an index >=
 * n_vertices; JPT_E_LIMIT: more than 2^25 triangles.  device_id >= 0: the kernels the rebuild launches, on that device; device_id < 0:
 * the same functions compiled for the host, sorted by std::sort. */
int jpt_debug_mesh_order(int device_id, const float *vertices3, uint32_t n_vertices, const uint32_t *indices, uint32_t n_tris,
                         uint32_t *codes_out /* may be NULL */, uint32_t *sorted_tris_out);

/* jpt_scene_pose_mesh's arithmetic alone, on one caller-made rig of n_vertices vertices (one surface's arrays, as jpt_surface_rig's;
 * bind_normals3 may be NULL: no normals, normals3_out is not written and normal_deltas must be NULL) and one pose.  The arguments are
 * checked as jpt_scene_set_mesh_rig and jpt_scene_pose_mesh check theirs (n_bones against the largest bone index included; n_vertices
 * == 0 or a NULL required array: JPT_E_INVALID).  device_id >= 0: the kernel jpt_scene_pose_mesh launches, on that device, over the rig
 * packed as jpt_scene_set_mesh_rig packs it; JPT_DEVICE_HOST_ONLY: the same functions in plain loops on the host. */
int jpt_debug_skin(int device_id, const float *bind_positions3, const float *bind_normals3 /* may be NULL */, uint32_t n_vertices,
                   const int32_t *bones, const float *weights, int32_t influences,
                   const float *position_deltas, const float *normal_deltas, int32_t n_blend_shapes,
                   const float *bone_transforms12, uint32_t n_bones, const float *blend_weights,
                   float *positions3_out, float *normals3_out);

/* jpt_encode's arithmetic alone, over n_texels caller-made float4 texels: rgb / divisor when divisor is not 1 (finite and > 0 required),
 * alpha as given or 1 (alpha_one != 0), then `format`; `out` takes n_texels * 8 (RGBA16F) or * 4 bytes.  n_texels = 0 succeeds and
 * writes nothing; more than 2^30 texels: JPT_E_LIMIT.  device_id >= 0: the kernel jpt_encode launches, on that device;
 * JPT_DEVICE_HOST_ONLY: the same functions compiled for the host, in a plain loop. */
int jpt_debug_encode(int device_id, const float *src4, uint64_t n_texels, float divisor, int32_t alpha_one, int32_t format, void *out);

/* ---- environment ------------------------------------------------------------------------------------------------------
 * The library READS these once per process (at the first jpt_create; gdpathtracing_amd/csrc/jpt_tuning.h) and never writes the
 * environment.  They are for tests, audits and profiling runs; an embedding application needs none of them -- everything a
 * host decides at run time has a call above (jpt_set_stream_priority, jpt_set_memory_policy, jpt_set_upload_mode, ...).
 *
 *   variable                  default   meaning
 *   JPT_SKY_CULL              1         0: every primary ray is traced (audits; the image is the same)
 *   JPT_WORKSPACE_BUDGET_MB   24576     most MiB one render's workspace may take before it is split into batches of frames
 *                                       (jpt_set_memory_policy overrides per context)
 *   JPT_PIPELINE              1         0: queued renders run one after another (per-kernel profiling: tools/pmc.sh, tools/diag.sh)
 *   JPT_PIPE_SLOTS            0         2..8: renders in flight (0: the library's rule -- 4, or 6 where six slot streams run side by side)
 *   JPT_GROUPS                0         1..4: frame groups of a blocking render (0: the library's rule; 1 for per-kernel profiling)
 *   JPT_UPLOAD_WALK           --        "given": every reference-layout upload is walked node for node as uploaded (JPT_UPLOAD_WALK_AS_GIVEN)
 *   JPT_SET_ASIDE_CAP         -1        records of the set-aside buffer (-1: 1/64 of the paths, at least 65 536; tests force 0)
 *   JPT_TAIL                  -1        a wave walks its last, long rays with all its lanes: -1 on scenes of >= 200 000 triangles, 0 never, 1 always
 *   JPT_TAIL_ROUNDS           128       ... from this many rounds after its block's queue ran dry
 *   JPT_TAIL_LANES            8         ... once it is down to this many rays
 *   JPT_LIB                   --        (Python binding only) path of the library to load instead of gdpathtracing_amd/libjpt_hip.so
 *
 * The HOST may want to export, before its first HIP call (see jpt_set_stream_priority above):
 *   GPU_MAX_HW_QUEUES               a pool of six per level: six renders in flight instead of four for queued renders (the HIP runtime's variable)
 *   HSA_ENABLE_IPC_MODE_LEGACY=0    multi-process runs (RCCL between ranks) on drivers that only support dmabuf IPC
 */

#ifdef __cplusplus
}
#endif
#endif /* JPT_H */
