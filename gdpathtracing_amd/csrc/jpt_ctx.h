// jpt_ctx.h -- the context behind the C ABI of include/jpt.h, with the helpers it is made of: private to the host layer
// (jpt_capi.cpp, jpt_scene.cpp, jpt_query.cpp, jpt_image.cpp, jpt_render.cpp, jpt_scene_update.cpp, jpt_lighting.cpp, jpt_primary.cpp, jpt_post.cpp,
// jpt_encode.cpp).
#pragma once
#include "../../include/jpt.h"

#include <chrono>
#include <map>

#include "jpt_builder.h"
#include "jpt_denoise.h"
#include "jpt_denoise_var.h"
#include "jpt_denoise_history.h"
#include "jpt_display.h"
#include "jpt_lightmap.h"
#include "jpt_meter.h"
#include "jpt_tlas_rebuild.h"
#include "jpt_variance.h"
#include "jpt_kernels.h"

namespace jpt {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t resize(size_t count)
    {
        if (count == n && (p || count == 0)) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const std::vector<T>& v, hipStream_t s)
    {
        hipError_t e = resize(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

// A grow-only pinned host buffer (hipHostMalloc), given back by its destructor or release()
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t reserve(size_t want)
    {
        if (bytes >= want) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

// A ring of pinned staging buffers, so that the host can queue device refits ahead of the device: a stage is written again once
// the work that last read it has run (its `copied` event)
constexpr int kRefitStages = 4;   // refits the host may queue before it has to wait for a copy to leave its buffer
struct StagingRing {
    PinnedBuf buf[kRefitStages];
    hipEvent_t copied[kRefitStages] = {};
    uint64_t seq = 0;
    ~StagingRing()
    {
        for (hipEvent_t e : copied)
            if (e) (void)hipEventDestroy(e);
    }
    // the next stage, of at least `bytes`, once the work that used it last has run
    hipError_t next(size_t bytes, int& st)
    {
        st = (int)(seq++ % (uint64_t)kRefitStages);
        hipError_t e = copied[st] ? hipEventSynchronize(copied[st]) : hipEventCreateWithFlags(&copied[st], hipEventDisableTiming);
        return e == hipSuccess ? buf[st].reserve(bytes) : e;
    }
};

// A read-back in two halves, so that the host does other work while the copy runs: begin queues the copy into a pinned buffer of its
// own on the caller's stream, wait blocks until it has landed.  One copy in flight at a time (`pending`; the owner refuses a second).
struct SplitReadback {
    PinnedBuf buf;
    hipEvent_t ev = nullptr;   // made at the first begin; follows the copy in flight
    bool pending = false;      // a begin has not been waited for yet
    size_t bytes = 0;          // what the copy in flight copies
    // `n` bytes at `src` -> buf behind everything queued on `s` so far (nothing is copied when n == 0)
    hipError_t begin(const void* src, size_t n, hipStream_t s)
    {
        hipError_t e = buf.reserve(n);
        if (e == hipSuccess && !ev) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess && n) e = hipMemcpyAsync(buf.p, src, n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        if (e != hipSuccess) return e;
        bytes = n;
        pending = true;
        return hipSuccess;
    }
    hipError_t wait()
    {
        const hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess) pending = false;
        return e;
    }
    void destroy()   // the event (the buffer is its destructor's)
    {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
};

// Several copies of the instance level (RefInstance + WideInstance arrays, TLAS tail of the four-child records): a refit writes a
// copy the renders in flight do NOT read, so the renders after a refit overlap with the renders before it.
constexpr int kInstanceSets = 8;   // as many as renders in flight can be: a queue of animation steps stays pipelined

// Every scene array on the device; the view the kernels take (jpt_ctx::ds) points into these (set_scene_view)
struct SceneBufs {
    // reference layout
    DevBuf<RefTriGeometry> tri_geom;
    DevBuf<ShadeTri> shade_tris;
    DevBuf<RefMaterial> materials;
    DevBuf<RefBvhNode> bvh;
    DevBuf<RefTlasNode> tlas;
    DevBuf<uint8_t> tex;
    // flattened layout
    DevBuf<WideNode> wblas, wtlas;
    DevBuf<WideTri> wtris;
    DevBuf<WideInstance> winst;
    DevBuf<WideNode4> nodes4;   // four-child records: BLAS part, then one TLAS tail per copy of the instance level (one index space)
    DevBuf<WideNodeQ> nodesq;   // their quantised form (jpt_nodeq.h), same indices: what the kernels walk
    // the instance level, one copy per kInstanceSets; copy 0 is the one uploads write (the reach records: JPT_BUILD_SAH)
    struct InstanceSet {
        DevBuf<RefInstance> inst;
        DevBuf<WideInstance> winst4;
        DevBuf<ReachInst> reach;
    } set[kInstanceSets];
    DevBuf<ReachTri> reach_tri;   // reach records per triangle
    DevBuf<float> cut_boxes;      // RefScene::inst_cut_boxes / inst_cut_range (device refits)
    DevBuf<uint32_t> cut_range;
    // the reference's own trees beside a native scene (ExactShadow): two-child records + the triangle map
    DevBuf<RefBvhNode> x_bvh;
    DevBuf<RefTriGeometry> x_tri_geom;
    DevBuf<RefInstance> x_inst;
    DevBuf<RefTlasNode> x_tlas;
    DevBuf<uint32_t> x_tri_native, x_native_ref, x_tri_leaf, x_subtree_end, x_tlas_parent, x_inst_leaf;
};

// One render in flight (jpt_render_async): its stream, its workspace and the events that order it.  Slot 0's workspace is
// also the one renders on the context's own stream use.
struct PipeSlot {
    hipStream_t stream = nullptr;
    hipEvent_t ev_paths_done = nullptr, ev_acc_done = nullptr;
    bool acc_done_valid = false;   // ev_acc_done follows the last accumulation that read `workspace`
    uint64_t refit_seen = 0;       // the refit (SceneUpdates::refit_wait_seq) the slot's stream has last waited for
    DevBuf<char> workspace;
};

// What the context holds of how its renders are planned, launched, pipelined and timed: written and read by the render entry points, the
// plan and the policy calls (jpt_render.cpp).  The rest of the host layer only tells it that a workspace was touched behind the
// pipeline's back (workspaces_touched: jpt_set_stream, the lighting's table kernels) and makes and gives back its events (jpt_create,
// jpt_destroy).  Render pipelining (jpt_render_async): consecutive asynchronous renders run their path kernels on the slots' streams with
// their own workspaces, so one render's launch tails overlap the next render's kernels; the accumulation kernels are ordered on the
// context's stream.
struct RenderPipe {
    // the render's event pair, around its launches on the context's stream: their distance is last_render_ms, and ev1 is also what
    // pipeline_idle asks (completed: nothing of this context is in flight)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the pipeline slots and the frame groups' helper streams, all made on first use
    static constexpr int kPipeSlots = 8;   // the most; the rule is 4, or 6 where six of the slots' streams run side by side (six_queues_probe)
    PipeSlot slot[kPipeSlots];
    Wf2Streams group_streams;                 // helper streams / events of the frame groups (launch_wf2_render)
    bool aux_borrowed[kMaxGroups - 1] = {};   // group_streams.aux_stream[k] is slot[k].stream (ensure_group_streams): not destroyed on its own
    // the plan's memory (plan_launch)
    int six_queues = -1;       // -1: not probed yet; 0 / 1
    int last_pipe_slots = 0;   // jpt_renders_in_flight
    uint64_t async_seq = 0;    // counts the queued renders (jpt_set_memory_policy starts it over): the next one's slot is async_seq % slots
    int idle_streak = 0;       // queued renders in a row that found nothing in flight
    // the host's policy
    int32_t slot_priority = JPT_STREAM_PRIORITY_DEFAULT;   // jpt_set_stream_priority
    int32_t max_slots = 0;                                 // jpt_set_memory_policy: renders in flight (0: the library's rule)
    uint64_t workspace_budget = 0;                         // ... and bytes per workspace (0: tuning().workspace_budget_mb)
    // what the last render left for the statistics
    std::vector<uint32_t> h_qcount;         // per-bounce queue sizes of the last wavefront render
    std::vector<hipEvent_t> trace_events;   // pairs around each wf_trace launch of the last render (jpt_ctx::kernel_timing)
    int32_t trace_events_used = 0;
    // the tiles' sky cells (launch_sky_tiles): a function of the camera, the image size and the partition -- made when one of them
    // changes, read by every accumulation until then
    DevBuf<uint32_t> d_sky_tiles;
    RefCamera sky_tiles_camera;
    int32_t sky_tiles_key[5] = {0, 0, 0, 0, 0};   // width, height, local_rows, rank, world
    bool sky_tiles_valid = false;

    // a slot's workspace (every slot's) was written or read outside the pipeline's own order: its ev_acc_done says nothing any more
    void workspace_touched(int k) { slot[k].acc_done_valid = false; }
    void workspaces_touched() { for (PipeSlot& ps : slot) ps.acc_done_valid = false; }
    hipError_t drain_slots();      // waits for every slot stream that exists; the first error
    void release_streams();        // drains and destroys the slots' streams and the helper streams; the next render that needs them makes new ones
    hipError_t create_events();    // ev0 and ev1 (jpt_create)
    void destroy();                // every event and stream above, once the context's stream has run dry (jpt_destroy)
};

// The launch shape of one render: where it runs, in how many frame groups, with how many segments per tracing block.
struct LaunchPlan {
    enum Route { kReference, kStream, kSlot } route = kReference;   // the reference-layout kernel / the context's stream / a pipeline slot
    int slot = 0, slots = 0;    // kSlot: the slot, and how many there are
    int groups = 1;             // frame groups (launch_wf2_render)
    int chain = 1;              // wf2_trace: consecutive segments per block
};
// What plan_launch asks of the device, each only where a rule reaches it (their side effects are part of the rules).
struct PlanDevice {
    bool (*six_queues)(jpt_ctx*);                // six of the slots' streams run side by side (six_queues_probe)
    bool (*idle)(jpt_ctx*);                      // nothing of this context is in flight (pipeline_idle)
    bool (*slot_stream)(jpt_ctx*, int slot);     // the slot's stream and events exist, made if need be (ensure_pipe_slot)
    int (*group_streams)(jpt_ctx*, int groups);  // helper streams there are for `groups` frame groups (ensure_group_streams)
};
// Every rule of a render's launch shape, in one place (jpt_render.cpp; declared here for tests/cpp/plan_launch_test.cpp, which passes a
// PlanDevice of its own).  fp: the render's frame_params; r: its sky cull and lighting.
LaunchPlan plan_launch(jpt_ctx* c, const FrameParams& fp, const Wf2Render& r, bool counted, bool blocking, const PlanDevice& dev);

// The temporal pass's state (JPT_DENOISE_TEMPORAL): written by jpt_set_temporal_params and the render that runs the pass (jpt_render.cpp),
// dropped by everything that starts its history over (restart), read by jpt_read_accum_f32.
struct TemporalState {
    RefTemporalParams temporal;
    bool temporal_set = false, hist_valid = false;
    DevBuf<float4> d_hist1, d_hist2;   // frameBuffer1 / frameBuffer2 of temporal_reprojection.glsl:16-17
    float4* hist_written = nullptr;    // the one the last temporal pass wrote
    // the history images start from zero at the next pass (a new TemporalReprojection object), and there is nothing to read until then
    void restart() { hist_valid = false; hist_written = nullptr; }
};

// What the context holds of its renders' lighting: written by the setters, read by lighting_bound and resolve_lighting (all in
// jpt_lighting.cpp), which turn it into the one value the renders take (Lighting, jpt_kernels.h)
struct LightingState {
    // the environment map (jpt_set_environment uploads it, jpt_set_sky writes it in place with a kernel): the context's, like its params
    DevBuf<float4> d_env;
    bool env_set = false;
    int32_t env_w = 0, env_h = 0;
    float env_rot[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float env_intensity = 1.0f;
    // the map's importance sampling (jpt_set_environment_sampling): the mode, also the context's, and the map's tables -- built once per
    // map while the mode is JPT_ENV_SAMPLING_MIS, then kept until the map changes
    int32_t env_sampling = JPT_ENV_SAMPLING_BRDF;
    DevBuf<float> d_env_cond, d_env_marg;   // h rows of w conditional CDF entries; the marginal CDF's h entries, then the total
    bool env_tables = false;
    float env_total = 0.0f;
    // importance sampling of the emissive triangles (jpt_set_light_sampling): the mode, the context's like the map's; the emitters
    // (instance, triangle pairs from c->scene.ref, host) and their device tables -- both made at the first render that needs them after
    // the scene changed (light_cand_stale: its instances or materials; light_table_stale: also its geometry, refits included)
    int32_t light_sampling = JPT_LIGHT_SAMPLING_BRDF;
    std::vector<uint32_t> light_cand_h;
    bool light_cand_stale = true, light_cand_uploaded = false, light_table_stale = true;
    DevBuf<uint32_t> d_light_cand;
    DevBuf<float4> d_light_tri;
    DevBuf<float> d_light_cdf, d_light_marg;   // per emitter; the marginal CDF's n_blocks entries, then the total power
    // material extensions (jpt_set_material_extensions): the flags, the context's like the modes; and whether some material of the
    // host's mirror (c->scene.ref.materials) has a sanitised transmission > 0, scanned whenever the materials may have changed
    uint32_t material_ext = JPT_MATERIAL_EXT_NONE;
    bool transmissive_materials = false;
};
// The scene changed: the emitter tables are rebuilt at the next render that samples them -- and the emitter list too when the
// instances or materials may have changed (`listed`: the materials are then scanned for a transmissive one as well); a refit or a
// mesh update moves the geometry only.  Costs nothing else.
void lights_stale(jpt_ctx* c, bool listed);
// The lighting a render of `c` would take now, for sizing: kind and miss model, no tables, no side effect.  A bound: while the
// emitter list is stale the answer is kEmitters whenever the mode asks for them (resolve_lighting decides).
Lighting lighting_bound(const jpt_ctx* c);
// The lighting of one render of `c`, once it is validated; makes the emitter tables on the context's stream when they are stale.
int resolve_lighting(jpt_ctx* c, Lighting& out);

// What the context holds of where its renders' paths start: written by the setters, read by resolve_primary and view_now (all in
// jpt_primary.cpp), which turn it into the one value the renders take (PrimaryRays, jpt_kernels.h)
struct PrimaryState {
    float lens_radius = 0.0f, lens_focus = 1.0f;   // jpt_set_lens: the context's, like the sampling modes; radius 0 is the pinhole
    int32_t camera_model = JPT_CAMERA_PINHOLE;     // jpt_set_camera_model: the context's, like the lens
    // jpt_set_bake_texels / jpt_bake_begin: the context's, like the environment map; present images make every render a bake render.
    // The rasteriser's winner image and staged surface (jpt_bake_add_surface) are grow-only
    DevBuf<float4> d_bake_pos, d_bake_nrm;
    int32_t bake_w = 0, bake_h = 0;
    DevBuf<uint32_t> d_bake_winner;
    DevBuf<char> d_bake_in;
    bool has_bake() const { return d_bake_nrm.p != nullptr; }
    // jpt_set_probes: the context's, like the bake images; present probes make every render a probe render (probe_w x probe_h pixels).
    // jpt_probe_project's own buffers: the quadrature table of (probe_tw, probe_th, table_flags) and the coefficients, 144 B per probe;
    // sh_valid: they hold a projection of the probes and the size as they are now
    DevBuf<float> d_probe_pos;
    int32_t probe_n = 0, probe_tw = 0, probe_th = 0, probe_per_row = 0, probe_w = 0, probe_h = 0;
    DevBuf<float> d_probe_table;
    int32_t table_tw = 0, table_th = 0, table_flags = -1;
    DevBuf<float4> d_probe_sh;
    bool sh_valid = false;
    bool has_probes() const { return d_probe_pos.p != nullptr; }
    ProbeDev probe_dev() const { return make_probe_dev(d_probe_pos.p, probe_n, probe_tw, probe_th, probe_per_row); }
    // jpt_set_reflection_probes: the context's, like the probes; present reflection probes make every render a cube render (cube_w x
    // cube_h pixels).  jpt_set_reflection_params: the context's (refl_levels 0: every level down to 1 x 1).  jpt_reflection_prefilter's
    // own buffers: the sample tables of (table_face, table_levels, table_samples), the source chain and the output chain (jpt_reflection.h);
    // refl_valid: the output chain holds refl_made levels of the probes and the size as they are now.  refl_ev: three events around the
    // two steps of the last jpt_reflection_prefilter under jpt_set_kernel_timing (refl_timed), made at the first such call.
    DevBuf<float> d_cube_pos;
    int32_t cube_n = 0, cube_face = 0, cube_per_row = 0, cube_w = 0, cube_h = 0;
    int32_t refl_levels = 0, refl_samples = kReflSamplesDefault;
    DevBuf<float4> d_refl_table;
    DevBuf<uint8_t> d_refl_lvl;
    uint32_t refl_count[kReflLevelsMax] = {};
    int32_t table_face = 0, table_levels = 0, table_samples = 0;
    DevBuf<float4> d_refl_chain, d_refl_out;
    int32_t refl_made = 0;
    bool refl_valid = false;
    hipEvent_t refl_ev[3] = {nullptr, nullptr, nullptr};
    bool refl_timed = false;
    bool has_cubes() const { return d_cube_pos.p != nullptr; }
    CubeDev cube_dev() const { return make_cube_dev(d_cube_pos.p, cube_n, cube_face, cube_per_row); }
    // the levels a jpt_reflection_prefilter of the probes makes now
    int32_t refl_levels_now() const { return refl_levels ? refl_levels : cube_log2(cube_face) + 1; }
    void destroy()   // refl_ev (jpt_destroy)
    {
        for (hipEvent_t& e : refl_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};
// Where the paths of one render of `c` start, once it is validated: the one of the six sources the context's state names, with the
// others zeroed; kPinhole with DEBUG_STEPS, which ignores the lens, the model, the images and the probes as it ignores lighting.  In
// this order -- bake images: JPT_E_STATE when their size is not the render's, with a lens radius > 0, a model other than the pinhole
// or the temporal pass (probes beside them are ignored: refused or rendered as a bake); reflection probes: JPT_E_STATE beside bake images or probes, then the same four refusals; probes: the same four refusals; a lens radius > 0: JPT_E_STATE with the temporal pass, a basis that is not finite or a model other than the
// pinhole; a model other than the pinhole: JPT_E_STATE with the temporal pass, EQUIRECT's basis or PROJECTIVE's ivp not finite.
int resolve_primary(jpt_ctx* c, PrimaryRays& out);
// The view of an entry point that takes it without rendering (`call`: jpt_denoise's guides, jpt_query_pixels' picking rays): the
// context's model seen through its camera as both are now -- no render's refusals apply.  JPT_E_STATE while the context holds bake
// images, probes or reflection probes (`rays`: what the call's rays are, for the message).
int view_now(jpt_ctx* c, const char* call, const char* rays, CamModelDev& out);
// What the context holds of the image itself: the framebuffers of its rows and their sizes, how often the progressive sum started over, the
// image assembled from every rank's piece, and the read-backs' staging (jpt_image.cpp).  Written by jpt_set_params / jpt_set_partition
// (alloc_framebuffers), the renders (jpt_render.cpp: the buffers, depth_valid), the two jpt_assemble_* calls and restart_sum; read by
// every post stage (jpt_post.cpp, jpt_primary.cpp, jpt_encode.cpp: d_accum) and every read-back.  The partition itself and the
// progressive count stay in jpt_ctx beside width and height (rank, world, local_rows, frame_count): a render's FrameParams are made
// of them, and tests/cpp/plan_launch_test.cpp sets them there.
struct ImageSource {
    const void* p;
    bool whole;   // p holds the whole image (else: the context's rows)
};
struct ImageState {
    // the partition's sizes (jpt_ctx::rank / world / local_rows are the renders' parameters, beside width and height: the context
    // renders the strips rank, rank + world, ... into local_rows rows, rows_of_rank).  Every rank's buffers have the size of the largest
    // rank's share, so that a gather sees equal pieces: piece_rows rows, piece_px pixels.  local_rows and these two are
    // alloc_framebuffers', which runs whenever the resolution or the partition changes.
    int32_t piece_rows = 0;
    size_t piece_px = 0;
    // framebuffers (piece_px each; the first local_rows rows are the context's)
    DevBuf<float4> d_accum;
    DevBuf<uint32_t> d_ldr;
    DevBuf<float> d_depth;
    bool depth_valid = false;      // d_depth holds the last render's depth image
    // the progressive count is jpt_ctx::frame_count (every render's FrameParams start from it); only restart_sum and the renders write it
    uint64_t accum_restarts = 0;  // how often the accumulation started over or was re-positioned (what a history call of jpt_denoise remembers)
    // assembled full image on the gathering rank
    DevBuf<float4> d_full_accum;
    DevBuf<uint32_t> d_full_ldr;
    bool assembled = false;        // d_full_accum + d_full_ldr hold the whole image (jpt_assemble_from_ranks)
    bool assembled_ldr = false;    // d_full_ldr only (jpt_assemble_ldr_from_ranks)
    // the read-backs' staging
    PinnedBuf h_read_pinned;       // blocking read-backs (staged_read; the ray queries and jpt_read_denoise_history_f32 borrow it)
    SplitReadback ldr_read;        // the split read-back of the display image (jpt_readback_ldr_begin / _end)
    bool readback_full = false;    // the read-back in flight copies the assembled image (else: this context's rows)

    // the display image (the sum) a read-back reads now: the assembled one while there is one
    ImageSource display_now() const
    {
        const bool whole = assembled || assembled_ldr;
        return {whole ? (const void*)d_full_ldr.p : d_ldr.p, whole};
    }
    ImageSource sum_now() const { return {assembled ? d_full_accum.p : d_accum.p, assembled}; }
    void destroy() { ldr_read.destroy(); }   // the split read-back's event (jpt_destroy)
};
// The one place that says what starts over when the progressive sum does, and for whom.  Every row drops the assembled image
// (assembled = assembled_ldr = false): it is of frames that are no longer the sum's.
//   how               caller                                      frame_count   accum_restarts   stats.frames   temporal history   post stages
//   kSumReset         jpt_accum_reset                             0             ++               0              restarted          --
//                     jpt_set_denoising_mode, on a change only
//   kSumPositioned    jpt_set_progressive_frame_count(n)          n - 1         ++               n - 1          kept               --
//   kSumFramebuffers  alloc_framebuffers                          0             ++               kept           kept (*)           framebuffers_remade(false)
//   kSumRendered      do_render_batch (adds its frames itself)    kept          kept             kept           kept               --
// (*) jpt_set_params restarts the temporal history itself, on another size only.  `count`: kSumPositioned's n - 1.
enum SumRestart { kSumReset, kSumPositioned, kSumFramebuffers, kSumRendered };
void restart_sum(jpt_ctx* c, SumRestart how, uint32_t count = 0);
// The partition's arithmetic (declared here for tests/cpp/image_rows_test.cpp): the rows of `rank`'s strips; the largest rank's share;
// a rank's rows, in the order of its buffers, to their image rows of `out` (px_bytes per pixel), on the host
int32_t rows_of_rank(int32_t height, int32_t rank, int32_t world);
int32_t max_rows_of_any_rank(int32_t height, int32_t world);
void scatter_rows(const char* local, char* out, int32_t width, int32_t height, int32_t rank, int32_t world, size_t px_bytes);
// Blocking read-backs: device -> the context's pinned read buffer (image.h_read_pinned), on the context's stream (jpt_image.cpp) ...
int staged_read(jpt_ctx* c, const void* src, size_t bytes);
// ... and on to the caller's memory: `bytes` at `out` (nothing is copied when bytes == 0)
int read_out(jpt_ctx* c, const void* src, size_t bytes, void* out);
// ... of an image of `comps` elements of `elem` bytes per pixel: `src` holds the whole image (`whole`), or the context's rows, which are
// scattered to their image rows of a zeroed `out` when the context is a partition (world > 1)
int read_rows_out(jpt_ctx* c, const void* src, size_t elem, int comps, bool whole, void* out);
// ... whose pinned buffer is given back whenever the framebuffers are re-made, and by jpt_set_memory_policy (jpt_render.cpp)
void release_read_staging(jpt_ctx* c);

// What the context holds of its post stages, the calls that read the progressive sum on the context's stream and keep what they make in
// buffers of their own: written and read by those calls and their read-backs (jpt_post.cpp; jpt_encode.cpp reads three of the images)
struct PostState {
    // jpt_denoise: the context's parameters, and its own images -- made at the first jpt_denoise at a resolution, kept until
    // jpt_set_params names another size; dn_valid: they hold the result of a jpt_denoise at the current resolution
    AtrousParams dn_params;
    DevBuf<float4> d_dn_pos, d_dn_nrm, d_dn_alb, d_dn_ping, d_dn_pong;
    DevBuf<uint32_t> d_dn_ldr;
    bool dn_valid = false;
    // jpt_set_denoise_variance: the context's parameters (dn_var.enable: the switch), and the plane of the variance the last pass leaves
    // (jpt_denoise_var.h; 4 B per pixel) -- made at the first guided jpt_denoise at a resolution, kept as jpt_denoise's images are;
    // dn_var_valid: the images hold the result of a guided jpt_denoise
    AtrousVarParams dn_var;
    DevBuf<float> d_dn_var;
    bool dn_var_valid = false;
    // jpt_set_denoise_history: the context's parameters (dn_hist.enable: the switch), and the stage's own images (jpt_denoise_history.h) --
    // two history sets of three planes each ((m, N), (n, S), position_t: the stage keeps its own copies of the guides, so a jpt_denoise
    // without history in between does not touch them) and the (m, v_0) image the filter reads, 112 B per pixel, made at the first
    // history call at a resolution; dh_cur: the set the last history call wrote, dh_have: it holds one (dropped by
    // jpt_denoise_history_reset, another size, switching enable), seen from dh_camera; dh_called / dh_restarts: a history call has
    // consumed the frames of accumulation restart dh_restarts (ImageState::accum_restarts); dh_read: d_dh_iv and set dh_cur hold a
    // history call's result at the current resolution (jpt_read_denoise_history_f32)
    HistoryParams dn_hist;
    DevBuf<float4> d_dh_set[2][3], d_dh_iv;
    int dh_cur = 0;
    bool dh_have = false, dh_called = false, dh_read = false;
    uint64_t dh_restarts = 0;
    RefCamera dh_camera;
    // jpt_bake_finish: the context's parameters, and its own images (two guides, a colour ping and pong: 64 B per texel) -- made at
    // the first jpt_bake_finish at a size, kept until jpt_set_params names another size or a call writes the bake images
    // (lightmap_release); lm_result: the one of ping / pong that holds the lightmap of a jpt_bake_finish at the current size and images
    LightmapParams lm_params;
    DevBuf<float4> d_lm_xg, d_lm_ng, d_lm_ping, d_lm_pong;
    const float4* lm_result = nullptr;
    // jpt_set_bake_directional: the switch, and the three moment planes a bake render adds to (jpt_bake_dir.h; 48 B per texel of the
    // context's rows) -- made by the first bake render with the switch on at a size (ensure_bake_dir), given back when the switch goes
    // off or the bake images are freed (bake_dir_release); bake_dir_valid: a bake render has written them at the current size.
    // jpt_bake_finish_directional: guides and working images of its own (jpt_bake_finish's lightmap stays what it is) and the three
    // finished planes, 112 B per texel in all, kept and given back as jpt_bake_finish's are (lmd_release); lmd_valid as lm_result.
    bool bake_dir = false;
    DevBuf<float4> d_bake_dir;
    bool bake_dir_valid = false;
    DevBuf<float4> d_lmd_xg, d_lmd_ng, d_lmd_ping, d_lmd_pong, d_lmd_out;
    bool lmd_valid = false;
    // jpt_display: the context's parameters, and its own buffers -- the two images made at the first jpt_display at a resolution,
    // the pyramid (six levels' worth) at the first one with bloom, kept until jpt_set_params names another size; disp_valid: the
    // images hold the result of a jpt_display at the current resolution
    DisplayParams disp_params;
    DevBuf<float4> d_disp_f32, d_disp_pyramid;
    DevBuf<uint32_t> d_disp_ldr;
    bool disp_valid = false;
    // jpt_meter: the context's parameters and the auto-exposure switch of jpt_display, and its own buffers -- the published bins, the
    // working sets (kMeterBinWords) and the state record, made at the first jpt_meter, kept until jpt_destroy; meter_valid: the record
    // holds the state a jpt_meter left since the last reset (jpt_meter_reset, jpt_set_params with another size), so the next jpt_meter
    // is not a FIRST one
    MeterParams meter_params;
    bool auto_exposure = false;
    DevBuf<uint32_t> d_meter_bins;
    DevBuf<MeterState> d_meter_state;
    bool meter_valid = false;
    // jpt_set_variance: the switch, and the plane of second moments every render adds to (jpt_variance.h; 16 B per pixel of the
    // context's rows) -- made by the first render with the switch on at a size (ensure_variance), given back when the switch goes off
    // (variance_release); variance_valid: a render has written it.  jpt_noise_estimate: the context's parameters, and its own buffers --
    // the tile map (4 B per 8 x 8 tile), the published bins and the working sets (kNoiseBinWords words, 17.3 KB) and the 32-byte
    // record, made at the first jpt_noise_estimate at a size; noise_valid: they hold the result of one at the current size.
    bool variance = false;
    DevBuf<float4> d_variance;
    bool variance_valid = false;
    NoiseParams noise_params;
    DevBuf<float> d_noise_tiles;
    DevBuf<uint32_t> d_noise_bins;
    DevBuf<NoiseResult> d_noise_result;
    bool noise_valid = false;

    void lightmap_release();   // jpt_bake_finish's images and result, and lmd_release
    void lmd_release();        // jpt_bake_finish_directional's images and result
    void bake_dir_release() { d_bake_dir.release(); bake_dir_valid = false; }
    void history_drop() { dh_have = dh_read = false; }   // the next history call starts without history (the planes stay)
    void variance_release() { d_variance.release(); d_noise_tiles.release(); variance_valid = noise_valid = false; }   // the plane and the tile map
    // The one place that says what re-made framebuffers do to this state (alloc_framebuffers: the plane and the estimate are of frames
    // that are gone) and, `resized`, what another image size does on top (jpt_set_params): every image of that size is given back and
    // every result of that size forgotten.  sized_buffers: whether one of the buffers it then frees exists -- work on the context's
    // stream may still use it, so the caller waits for the stream first.
    bool sized_buffers() const { return d_dn_ping.p || d_dh_iv.p || d_lm_ping.p || d_lmd_out.p || d_disp_f32.p || d_disp_pyramid.p; }
    void framebuffers_remade(bool resized);
};
// What a render refuses with the directional planes (the variance plane) switched on, and the planes (the plane) at the size of the
// context's rows for it: do_render_batch's (jpt_post.cpp)
int check_bake_directional(jpt_ctx* c);
int ensure_bake_dir(jpt_ctx* c);
int check_variance(jpt_ctx* c);
int ensure_variance(jpt_ctx* c);
// The refusals every call that reads the progressive sum opens with, in their order: a denoising mode other than progressive ("<call><what>:
// the denoising mode must be ..."), DEBUG_STEPS (`steps`: the call's own sentence), a partition ("<call> needs the whole image ...<whole>")
// and, unless `host_only` is null, a host-only context, in the call's own words.  sum_ready: no jpt_set_params, no frame since the reset.
int reads_sum(jpt_ctx* c, const char* call, const char* what, const char* host_only, const char* whole = "", const char* steps = nullptr);
int sum_ready(jpt_ctx* c, const char* call);

// What the context holds of jpt_encode: written and read by that call, its read-backs and its timing (jpt_encode.cpp).  The buffer is its
// own, grow-only and kept until jpt_destroy -- a snapshot that no other call writes; valid: it holds the texels `info` describes.
// ev: two events around the last jpt_encode's kernel under jpt_set_kernel_timing (timed), made at the first such call.  read: the split
// read-back of the buffer (jpt_readback_encoded_begin / _end), with staging of its own beside the display image's.
struct EncodeState {
    DevBuf<char> d_encoded;
    jpt_encoded_info info = {};
    bool valid = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
    SplitReadback read;
    void destroy()   // the events (jpt_destroy)
    {
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        read.destroy();
    }
};

// What the context holds of the calls that change a committed scene on the device without a new commit (the refits, rebuilds, mesh updates,
// rigs and poses of jpt_scene_update.cpp, and its two debug readers).  The uploads (jpt_scene.cpp) put it back through host_uploaded; the
// renders read cur_set through the view, wait for ev_refit_done and refuse on refit_active / mesh_deformed.
struct SceneUpdates {
    // device refit of the instance level (jpt_scene_refit_tlas)
    StagingRing refit_stage;           // pinned staging for the transforms
    size_t tlas4_cap = 0;              // records reserved per TLAS tail
    int cur_set = 0;                   // which copy new renders read
    bool set_b_ready = false;          // copies 1.. exist and mirror the last host upload
    hipStream_t refit_stream = nullptr;
    hipEvent_t ev_set_retired[kInstanceSets] = {}, ev_refit_done = nullptr;
    bool set_retired_valid[kInstanceSets] = {};
    uint64_t refit_wait_seq = 0;
    DevBuf<uint32_t> d_tlas4_order, d_tlas4_levels;
    bool refit_active = false;         // the device's instance level is ahead of the host mirrors (and of the other kernels' arrays)
    bool cull_boxes_current = true;    // c->scene.wide.tlas_nodes4 holds the boxes of the copy new renders read (sky cull)
    std::vector<uint32_t> tlas4_order_h, tlas4_levels_h;   // the refit schedule, host copy
    // a new topology made on the device (jpt_scene_rebuild_tlas): the template of the scene's instance count with its schedule and the
    // sort's buffers, made at the first rebuild of that count and kept.  After a rebuild c->scene.wide.tlas_nodes4 / tlas_root4 / stack_need4
    // and the schedule's host copy above are the template's, and the refits run over tmpl_order / tmpl_levels (topo_rebuilt), until
    // the next upload.  topo_gen counts the rebuilds since the last upload; set_topo_gen[k]: the one whose topology the TLAS tail of
    // copy k holds (a refit into a copy that is behind first copies the current copy's tail: queue_instance_refit).
    TlasTemplate tlas_tmpl;
    std::vector<uint32_t> tmpl_order_h, tmpl_levels_h;
    uint32_t tmpl_stack_need = 0;
    DevBuf<int32_t> d_tmpl_child;
    DevBuf<uint32_t> d_tmpl_order, d_tmpl_levels, d_tlas_sorted;
    DevBuf<uint64_t> d_tlas_sort_keys;
    bool topo_rebuilt = false;
    uint32_t topo_gen = 0, set_topo_gen[kInstanceSets] = {};
    // deforming committed meshes on the device (jpt_scene_update_mesh).  Per mesh: its records in dev.nodes4 and its schedule
    // (refit4_schedule), made at the first update after an upload
    struct MeshRefit {
        bool has_tree = false;              // an instance names the mesh and it has triangles: the device holds its tree
        int32_t root4 = 0;                  // its root reference in dev.nodes4
        uint32_t bvh_root = 0;              // its root in dev.bvh (RefScene::mesh_roots)
        uint32_t tri_first = 0, n_tris = 0;
        uint32_t rec_first = 0, n_recs = 0;  // the span of dev.nodes4 its records occupy
        uint32_t level_first = 0, n_levels = 0;   // its level starts: mesh_levels_h[level_first .. level_first + n_levels]
        bool rebuilt = false;               // jpt_scene_rebuild_mesh gave it a region: root4 / rec_first / n_recs name the region, the levels are mesh_regions[mesh]'s (level_first 0)
    };
    // A new topology made on the device (jpt_scene_rebuild_mesh).  Per rebuilt mesh a region of dev.nodes4 / nodesq BEHIND the TLAS tails
    // (the template of its triangle count needs more records than the commit's tree has), reserved at the mesh's first rebuild and kept
    // until the next whole upload, with the template's child words, its schedule (absolute record indices) and level starts; the old range
    // is no longer referenced.  mesh_need: the stack need of every mesh's tree
    // as it is now (made at the first rebuild: c->scene.wide.stack_need4 is the TLAS need + 1 + the largest of them).  d_mesh_sort: the sort's
    // working set, of the largest mesh rebuilt so far (jpt_mesh_rebuild.h: mesh_sort_words).
    struct MeshRegion {
        DevBuf<int32_t> d_child;
        DevBuf<uint32_t> d_order, d_levels;
        std::vector<uint32_t> levels_h;
    };
    std::map<uint32_t, MeshRegion> mesh_regions;
    std::vector<uint32_t> mesh_need;
    DevBuf<uint32_t> d_mesh_sort;
    std::vector<MeshRefit> mesh_refit;
    bool mesh_refit_ready = false;
    std::vector<uint32_t> mesh_order_h, mesh_levels_h;
    DevBuf<uint32_t> d_mesh_order, d_mesh_levels, d_tri_vidx;
    DevBuf<char> d_mesh_in;                  // the staged update: bounds header, vertices, normals
    StagingRing mesh_stage;            // pinned staging for the updates (header, vertices, normals, transforms)
    hipEvent_t ev_mesh_drain = nullptr;
    bool mesh_deformed = false;   // a mesh was deformed on the device: the host mirrors (c->scene.ref, c->scene.wide) are stale until the next upload
    // posing committed meshes on the device (jpt_scene_set_mesh_rig / jpt_scene_pose_mesh): per rigged mesh the rig's layout and, when
    // an instance names the mesh, its block on the device (jpt_kernels_skin.hip); dropped by jpt_scene_begin and every upload
    struct MeshRig {
        SkinRigInfo info;
        DevBuf<char> d_rig;   // empty for a mesh no instance names
    };
    std::map<uint32_t, MeshRig> mesh_rigs;
    // The one place that says which state a host upload puts back (finish_upload, jpt_scene.cpp): of the whole scene `w` (`whole`) or of
    // its instance level only, which leaves what is known of the meshes.  A scene without four-child records uploads no tails:
    // tlas4_cap and cull_boxes_current then stay what the scene before it left.
    void host_uploaded(bool whole, const WideScene& w)
    {
        cur_set = 0;
        set_b_ready = false;  // the instance arrays of the other copies are made (again) by the next refit
        for (bool& v : set_retired_valid) v = false;
        // every tail gets the host's topology again: the refits run over its schedule until the next jpt_scene_rebuild_tlas
        topo_rebuilt = false;
        topo_gen = 0;
        for (uint32_t& g : set_topo_gen) g = 0;
        refit_active = false;
        if (whole) mesh_deformed = mesh_refit_ready = false;
        if (whole) mesh_need.clear();   // (upload_nodes4 makes the record arrays anew: the regions behind the tails are gone; drop_mesh_rigs freed their schedules)
        if (!w.instances4.empty() || !w.blas_nodes4.empty()) cull_boxes_current = true;
    }
    // the first record of copy k's TLAS tail in dev.nodes4 (upload_nodes4: the BLAS records, then one tail per copy)
    size_t tail_first(const WideScene& w, int k) const { return w.blas_nodes4.size() + (size_t)k * tlas4_cap; }
    // The refit stream and the events ensure_refit_stream and the mesh calls make, given back once the stream has run dry (jpt_destroy)
    void destroy_stream()
    {
        if (refit_stream) { (void)hipStreamSynchronize(refit_stream); (void)hipStreamDestroy(refit_stream); }
        for (hipEvent_t e : ev_set_retired) if (e) (void)hipEventDestroy(e);
        if (ev_refit_done) (void)hipEventDestroy(ev_refit_done);
        if (ev_mesh_drain) (void)hipEventDestroy(ev_mesh_drain);
    }
};
// The scene on the host: the builder of the last jpt_scene_begin, the scene in the reference's layout (ref) and flattened (wide), and what
// says which calls it admits.  Written by the entry points of jpt_scene.cpp and by move_instances (jpt_scene_update.cpp: the builder's
// transforms, tlas_dirty); read by every file of the host layer -- the renders and post stages ask device_ready, the lighting reads ref.
// The state, row by row as the code has it ("." stays; rigs: drop_mesh_rigs, the rigs and regions of SceneUpdates; ms: stats.last_build_ms;
// refit / deformed: upd.refit_active / upd.mesh_deformed, put back by host_uploaded, which a host-only context never reaches -- there both stay false):
//   call                                     building  host_ready  device_ready  from_commit  tlas_dirty  tree       upload_note   rigs     refit  deformed  ms
//   jpt_scene_begin                          true      .           .             .            .           .          .             dropped  .      .         .
//   jpt_scene_commit, accepted               false     true        true (1)      true         false       builder's  ""            dropped  false  false     written
//     refused by the builder                 . (true)  false       false         .            .           .          .             dropped  .      .         .
//     refused by validate_ref_scene          . (true)  false       false         .            .           builder's  .             dropped  .      .         .
//     refused as too deep (or by flatten)    false     false       false         true         .           builder's  ""            dropped  .      .         written
//   jpt_scene_upload_reference_layout
//     native                                 .         true        true (1)      false        false       REACH      "" (2)        dropped  false  false     written
//     as given                               .         true        true (1)      false        false       AS_GIVEN   why           dropped  false  false     written
//     refused before the arrays are taken    .         .           .             .            .           .          .             .        .      .         .
//     refused after, by validate_ref_scene   .         false       false         false        .           .          ""            dropped  .      .         .
//     refused after, as too deep / flatten   .         false       false         false        .           as above   as above      dropped  .      .         written
//   jpt_scene_share (the destination)        false     true        true (1)      source's     false       source's   source's      dropped  false  false     written
//     (the source, when from_commit and tlas_dirty or refit: jpt_scene_update_tlas below; refused: the destination is not touched)
//   jpt_scene_set_instance_transform         .         .           .             .            true        .          .             .        .      .         .
//   jpt_scene_update_tlas, nothing dirty     .         .           .             .            .           .          .             .        .      .         .
//     accepted                               .         .           .             .            false       .          .             .        false  .         written
//     refused by the builder                 .         false       false         .            .           .          .             kept     .      .         .
//     refused as too deep                    .         false       false         .            .           .          .             kept     .      .         written
//     refused by reflatten_tlas              .         .           .             .            .           .          .             .        .      .         written
//   jpt_scene_update_reference_tlas
//     accepted                               .         .           .             .            .           .          .             .        false  .         written
//     refused before the arrays are taken    .         .           .             .            .           .          .             .        .      .         . (3)
//     rejected and rolled back               .         true        true (1)      .            .           .          .             .        false  .         written
//     rolled back, the way back failed       .         false       false         .            .           .          .             kept     (4)    .         written
//   jpt_scene_refit_tlas, _rebuild_tlas      .         .           .             .            true        .          .             .        true   .         written
//     (without four-child records on the device: jpt_scene_update_tlas; a refusal after the device check -- the rebuild's limits, a device
//     error -- leaves tlas_dirty true and the builder's transforms set, and writes no ms)
//   jpt_scene_update_mesh, _rebuild_mesh,    .         .           .             .            .           .          .             . (5)    true   true      written
//   jpt_scene_pose_mesh, _pose_mesh_rebuild
// (1) false on a host-only context.  (2) or why the arrays are walked as given after all, with tree AS_GIVEN.  (3) the native route's
// refusal by native_instances_from_uploaded comes after t0 was taken and still writes nothing.  (4) whatever the failed upload left.
// (5) jpt_scene_rebuild_mesh adds the mesh's region.  A device error (JPT_E_DEVICE) leaves the flags of the step it
// stopped at: in an upload of the whole scene host_ready true and device_ready false, in one of the instance level both as they were.
struct HostScene {
    SceneBuilder builder;
    RefScene ref;
    WideScene wide;
    bool building = false;       // between jpt_scene_begin and the commit that is accepted (or refused too deep)
    bool host_ready = false;     // ref / wide hold a complete scene (also true on host-only contexts)
    bool device_ready = false;   // ... and jpt_ctx::dev holds it: what a render, a post stage and a query ask
    bool from_commit = false;    // the scene came from jpt_scene_commit: builder holds its meshes and transforms
    bool tlas_dirty = false;     // builder's transforms are ahead of ref's instance level
    int32_t tree = JPT_TREE_NONE;   // the JPT_TREE_* of the scene in ref (jpt_scene_tree_kind answers it once host_ready)
    int32_t upload_mode = JPT_UPLOAD_NATIVE_TREE;  // jpt_set_upload_mode
    // jpt_scene_upload_note and jpt_scene_ties_exact hand out their c_str(): they live as long as the context
    std::string upload_note;     // why the last reference-layout upload is walked as given (empty: it is not)
    std::string ties_note;       // why exact distance ties fall to the native tree's order (empty: they are decided exactly)
    // jpt_scene_set_materials / _set_textures, until the commit copies them into ref
    std::vector<RefMaterial> pending_materials;
    std::vector<uint8_t> pending_tex;
    int32_t pending_tex_res = 0, pending_layers = 0;

    // the kernels walk the four-child records of the native tree (the native builder's trees and native uploads); reference-exact and
    // as-given trees keep the two-child records so the kernels visit them node for node like main.glsl (event counters equal the oracle's)
    bool walks_nodes4() const { return tree == JPT_TREE_NATIVE_REACH || tree == JPT_TREE_NATIVE_WATERTIGHT; }
    // what a traversal of the scene in `wide` could need of the kernels' stack
    uint32_t stack_need() const { return walks_nodes4() ? wide.stack_need4 : wide.stack_need2; }
    void not_ready() { host_ready = device_ready = false; }   // (the rigs stay: scene_left, jpt_scene.cpp, is the whole transition)
};
// A tree deeper than the kernels' stack, refused where it is made (`after`: "", " after the TLAS update", " after the TLAS rebuild",
// " after the mesh rebuild"; jpt_scene.cpp, with the other transitions and refusals the scene's calls share)
int too_deep(jpt_ctx* c, uint32_t need, const char* after);
// host time since t0, for stats.last_build_ms (no scope guard: the early returns of the calls that time themselves write nothing)
inline double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// the view the kernels take (c->ds) of the scene's device arrays, with the instance level of the copy new renders read (jpt_scene.cpp)
void set_scene_view(jpt_ctx* c);
// the rigs of jpt_scene_set_mesh_rig, and the regions of jpt_scene_rebuild_mesh, leave with the scene they were set for, behind the refit stream (jpt_scene_update.cpp)
void drop_mesh_rigs(jpt_ctx* c);
// The refusals these calls open with: no context (JPT_E_INVALID), no scene from jpt_scene_commit ("<call><what>"); for the two trees a
// JPT_BUILD_REFERENCE_EXACT commit (`exact`: the call's sentence, null: "<call><what>" again); for kWatertightTree a JPT_BUILD_SAH commit (`sah`,
// likewise).  on_device, after the argument checks: a host-only context, in the call's words, and with `scene` "no scene on the device"
// (jpt_scene.cpp)
enum SceneNeed { kFromCommit, kNativeTree, kWatertightTree };
int needs_scene(jpt_ctx* c, SceneNeed need, const char* call, const char* what, const char* exact = nullptr, const char* sah = nullptr);
int on_device(jpt_ctx* c, const char* host_only, bool scene);

// jpt_query_rays / jpt_query_pixels (host forms, jpt_query.cpp): one chunk's rays, hits and occlusion bytes on the device, grow-only.  The
// host side of a chunk borrows the image's pinned read buffer (image.h_read_pinned): a query and a blocking read-back never overlap.
struct QueryState {
    DevBuf<char> d_query;
};

}  // namespace jpt

using namespace jpt;   // (jpt_ctx is the name include/jpt.h gives it: global)

struct jpt_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string error;

    HostScene scene;          // the builder, the scene on the host, its flags and notes (jpt_scene.cpp; the table: HostScene)

    // device scene
    SceneBufs dev;
    DeviceScene ds;

    // per-render state
    bool params_set = false, camera_set = false;
    int32_t width = 0, height = 0, max_bounces = 4, accum_mode = 0, sampler_mode = 0;
    int32_t rank = 0, world = 1, local_rows = 0;   // jpt_set_partition; local_rows: alloc_framebuffers' (jpt_image.cpp)
    RefCamera camera;
    uint32_t frame_count = 0;  // frames accumulated since reset (restart_sum, jpt_image.cpp)
    int32_t kernel_variant = JPT_KERNEL_WAVEFRONT;
    bool debug_steps = false;  // jpt_set_debug_steps: the shader's DEBUG_STEPS build, on the audit kernel
    uint32_t outputs = JPT_OUTPUT_DEPTH;   // jpt_set_outputs: which of main.glsl's images the renders produce beside the colour
    bool kernel_timing = false;   // jpt_set_kernel_timing: event pairs around the launches (pipe.trace_events, primary.refl_ev, enc.ev)
    DevBuf<DevCounters> d_counters;   // a counted render's event counters (made with the framebuffers, read into stats)

    // post-processing mode (PathTracingCamera::Denoising)
    int32_t denoise = JPT_DENOISE_PROGRESSIVE;

    ImageState image;         // the framebuffers and their sizes, the restart count, the assembled image and the read-backs' staging (jpt_image.cpp)
    RenderPipe pipe;         // the events, slots, streams, plan memory and policy of the renders (jpt_render.cpp)
    TemporalState reproj;     // the temporal pass's parameters and history images (jpt_render.cpp)
    LightingState lighting;   // the environment map, the emitters and their sampling modes (jpt_lighting.cpp)
    PrimaryState primary;     // the lens, the camera model, the bake images, the probes and the reflection probes (jpt_primary.cpp)
    PostState post;           // the parameters, buffers and validity flags of the calls that read the progressive sum (jpt_post.cpp)
    SceneUpdates upd;         // the copies, streams, schedules and flags of the calls that change a committed scene on the device (jpt_scene_update.cpp)
    EncodeState enc;          // jpt_encode's buffer, what it holds, its timing and its split read-back (jpt_encode.cpp)

    QueryState query;         // the host forms' staging on the device (jpt_query.cpp)

    jpt_stats stats;
};

static inline int fail(jpt_ctx* c, int code, const std::string& msg)
{
    if (c) c->error = msg;
    return code;
}

static inline int hip_fail(jpt_ctx* c, hipError_t e, const char* what)
{
    return fail(c, JPT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(c, expr)                                          \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) return hip_fail((c), e_, #expr);    \
    } while (0)
