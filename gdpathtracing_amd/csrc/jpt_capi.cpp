// jpt_capi.cpp -- the C ABI of include/jpt.h over the HIP kernels and the host builder: the context's life cycle and stream, the host
// scene and its uploads, the ray queries and the one-line setters (the rest of the ABI: the other host files named in jpt_ctx.h).
#include "jpt_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "jpt_tuning.h"

// The view the kernels take (c->ds) of the scene's device arrays (c->dev): the counts from c->ref / c->wide, the instance level the
// copy new renders read (cur_set).  Whether the tie shadow is usable and current (ds.x.ok, ds.x.tlas_current) is upload_shadow's.
void jpt::set_scene_view(jpt_ctx* c)
{
    const SceneBufs& b = c->dev;
    const SceneBufs::InstanceSet& is = b.set[c->upd.cur_set];
    const RefScene& r = c->ref;
    const WideScene& w = c->wide;
    DeviceScene& d = c->ds;
    const bool reach = !r.reach_tri.empty() && r.reach_tri.size() == r.tri_geom.size() && r.reach_inst.size() == r.instances.size();
    d.reach_tri = reach ? b.reach_tri.p : nullptr;
    d.reach_inst = reach ? is.reach.p : nullptr;
    d.ref_tri_geom = b.tri_geom.p;
    d.shade_tris = b.shade_tris.p;
    d.ref_materials = b.materials.p;
    d.ref_bvh = b.bvh.p;
    d.ref_instances = is.inst.p;
    d.ref_tlas = b.tlas.p;
    d.tex = b.tex.p;
    d.n_tris = (uint32_t)r.tri_geom.size();
    d.n_materials = (uint32_t)r.materials.size();
    d.n_ref_bvh = (uint32_t)r.bvh_nodes.size();
    d.n_instances = (uint32_t)r.instances.size();
    d.n_ref_tlas = (uint32_t)r.tlas_nodes.size();
    d.tex_res = r.tex_res;
    d.n_layers = r.n_layers;
    d.blas_nodes = b.wblas.p;
    d.wide_tris = b.wtris.p;
    d.tlas_nodes = b.wtlas.p;
    d.wide_instances = b.winst.p;
    d.tlas_root = w.tlas_root;
    d.n_blas_nodes = (uint32_t)w.blas_nodes.size();
    d.n_tlas_nodes = (uint32_t)w.tlas_nodes.size();
    d.use4 = walks_nodes4(c);
    d.stack_need4 = w.stack_need4;
    d.wide_instances4 = is.winst4.p;
    // upload_nodes4: the BLAS records, then the TLAS tail of each copy
    const bool any4 = !w.instances4.empty() || !w.blas_nodes4.empty();
    const size_t tail_base = c->upd.tail_first(w, c->upd.cur_set);
    d.nodes4 = any4 ? b.nodes4.p : nullptr;
    d.nodesq = any4 ? b.nodesq.p : nullptr;
    d.tlas_root4 = !any4 ? 0 : w.tlas_root4 >= 0 ? w.tlas_root4 + (int32_t)tail_base : w.tlas_root4;
    TieShadowDev& x = d.x;
    x.bvh = b.x_bvh.p;
    x.tri_geom = b.x_tri_geom.p;
    x.instances = b.x_inst.p;
    x.tlas = b.x_tlas.p;
    x.tri_native = b.x_tri_native.p;
    x.native_ref = b.x_native_ref.p;
    x.tri_leaf = b.x_tri_leaf.p;
    x.subtree_end = b.x_subtree_end.p;
    x.tlas_parent = b.x_tlas_parent.p;
    x.inst_tlas_leaf = b.x_inst_leaf.p;
}

namespace {

thread_local std::string g_create_error;

// the builder's mode for the scene's tree (an as-given upload: ReferenceExact; rebuild_instances only sees committed scenes)
BuildMode build_mode(const jpt_ctx* c)
{
    if (c->tree == JPT_TREE_NATIVE_REACH) return BuildMode::Sah;
    if (c->tree == JPT_TREE_NATIVE_WATERTIGHT) return BuildMode::SahWatertight;
    return BuildMode::ReferenceExact;
}

// Four-child records on the device: [ BLAS records | TLAS records ], internal child references of the TLAS part and
// the TLAS root shifted by the BLAS count.  The TLAS part has room for the largest TLAS of this instance count
// (<= one record per instance), so a TLAS update rewrites the tail only.
int upload_nodes4(jpt_ctx* c, bool tlas_only)
{
    const WideScene& w = c->wide;
    const size_t nb = w.blas_nodes4.size(), nt = w.tlas_nodes4.size();
    const size_t cap_t = std::max<size_t>(w.instances4.size(), std::max<size_t>(nt, 1));
    const size_t cap = nb + (size_t)kInstanceSets * cap_t;  // one TLAS tail per copy of the instance level (jpt_scene_refit_tlas)
    hipStream_t s = c->stream;
    if (w.instances4.empty() && nb == 0) return JPT_OK;
    auto quantised = [](const std::vector<WideNode4>& in) {
        std::vector<WideNodeQ> out(in.size());
        for (size_t i = 0; i < in.size(); i++) quantize_node4(in[i], out[i]);
        return out;
    };
    SceneBufs& b = c->dev;
    if (!tlas_only || b.nodes4.n < cap) {
        HIP_TRY(c, b.nodes4.resize(cap));
        HIP_TRY(c, b.nodesq.resize(cap));
        if (nb) {
            const std::vector<WideNodeQ> q = quantised(w.blas_nodes4);
            HIP_TRY(c, hipMemcpyAsync(b.nodes4.p, w.blas_nodes4.data(), nb * sizeof(WideNode4), hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(b.nodesq.p, q.data(), nb * sizeof(WideNodeQ), hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipStreamSynchronize(s));  // `q` is pageable host memory
        }
    }
    for (int copy = 0; copy < kInstanceSets; copy++) {
        const size_t base = nb + (size_t)copy * cap_t;
        std::vector<WideNode4> tail(w.tlas_nodes4);
        for (WideNode4& n : tail)
            for (int k = 0; k < 4; k++)
                if (n.child[k] >= 0) n.child[k] += (int32_t)base;
        const std::vector<WideNodeQ> qtail = quantised(tail);
        if (nt) HIP_TRY(c, hipMemcpyAsync(b.nodes4.p + base, tail.data(), nt * sizeof(WideNode4), hipMemcpyHostToDevice, s));
        if (nt) HIP_TRY(c, hipMemcpyAsync(b.nodesq.p + base, qtail.data(), nt * sizeof(WideNodeQ), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));  // `tail`, `qtail` are pageable host memory
    }
    c->upd.tlas4_cap = cap_t;
    // bottom-up schedule of the TLAS records, for refits on the device
    tlas4_refit_schedule(w, c->upd.tlas4_order_h, c->upd.tlas4_levels_h);
    HIP_TRY(c, c->upd.d_tlas4_order.upload(c->upd.tlas4_order_h, s));
    HIP_TRY(c, c->upd.d_tlas4_levels.upload(c->upd.tlas4_levels_h, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // pageable host vectors
    return JPT_OK;
}

// Why exact distance ties fall to the native tree's order, for jpt_scene_ties_exact (this used to be silent).  A
// tree of the reference's own -- uploads walked as given, JPT_BUILD_REFERENCE_EXACT -- needs no shadow: its walk IS the
// reference's.
void note_ties(jpt_ctx* c)
{
    const ExactShadow& x = c->ref.exact;
    c->ties_note.clear();
    if (walks_nodes4(c)) {
        if (c->ref.reach_tri.empty()) c->ties_note = "the scene has no reach records (JPT_BUILD_SAH_WATERTIGHT): the native tree's order decides";
        else if (x.instances.empty()) c->ties_note.clear();   // nothing to hit
        else if (!x.valid) c->ties_note = "the reference's TLAS of this scene could not be built (TLAS::build, bvh.cpp:264-317)";
        else if (!x.resolvable)
            c->ties_note = "the uploaded trees are not in the shape the restricted walk indexes: every BLAS numbered in pre-order "
                           "(left child = parent + 1, what build_recursive emits, bvh.cpp:108-185) and every instance in exactly one "
                           "TLAS leaf reachable from slot 0";
    }
}

// The shadow (the reference's own trees beside a native scene, ExactShadow) -> the device, for jpt_tie_walk.h.
// `instances_only`: the BLAS part is there already (a TLAS update).  Not having a shadow is not an error: exact distance
// ties are then decided by the order of the native walk.
int upload_shadow(jpt_ctx* c, bool instances_only)
{
    c->ds.x.ok = false;
    const ExactShadow& x = c->ref.exact;
    note_ties(c);
    if (!x.valid || !x.resolvable || !walks_nodes4(c) || c->ref.reach_tri.empty() || c->device < 0 || x.instances.empty())
        return JPT_OK;
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    if (!instances_only) {
        HIP_TRY(c, b.x_bvh.upload(x.bvh_nodes, s));
        HIP_TRY(c, b.x_tri_geom.upload(x.tri_geom, s));
        HIP_TRY(c, b.x_tri_native.upload(x.tri_native, s));
        HIP_TRY(c, b.x_native_ref.upload(x.native_ref, s));
        HIP_TRY(c, b.x_tri_leaf.upload(x.tri_leaf, s));
        HIP_TRY(c, b.x_subtree_end.upload(x.subtree_end, s));
    }
    HIP_TRY(c, b.x_inst.upload(x.instances, s));
    HIP_TRY(c, b.x_tlas.upload(x.tlas_nodes, s));
    HIP_TRY(c, b.x_tlas_parent.upload(x.tlas_parent, s));
    HIP_TRY(c, b.x_inst_leaf.upload(x.inst_tlas_leaf, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->ds.x.ok = true;
    c->ds.x.tlas_current = true;
    return JPT_OK;
}

// What both uploads end with on the device, of the `whole` scene or of its instance level: the one place that says a host upload
// happened (SceneUpdates::host_uploaded; a host-only context never leaves that state), then the four-child records, the shadow and the view
int finish_upload(jpt_ctx* c, bool whole)
{
    c->upd.host_uploaded(whole, c->wide);
    int rc = upload_nodes4(c, !whole);
    if (rc != JPT_OK) return rc;
    rc = upload_shadow(c, !whole);
    set_scene_view(c);
    return rc;
}

// host RefScene (+ flatten) -> device
int upload_scene(jpt_ctx* c)
{
    drop_mesh_rigs(c);   // (before anything can refuse the scene: no rig outlives the scene it was set for)
    lights_stale(c, true);
    std::string err;
    if (!flatten(c->ref, c->wide, err)) return fail(c, JPT_E_INVALID, "flatten: " + err);
    const bool use4 = walks_nodes4(c);
    if (use4) flatten4(c->wide);
    else {
        c->wide.blas_nodes4.clear();
        c->wide.tlas_nodes4.clear();
        c->wide.instances4.clear();
    }
    compute_stack_need(c->wide);
    {
        // the reference walks with two unchecked 64-entry stacks (main.glsl:272,307); here a deeper tree is an
        // error at upload time instead of undefined behaviour at render time
        const uint32_t need = use4 ? c->wide.stack_need4 : c->wide.stack_need2;
        if (need > trace_stack_capacity())
            return fail(c, JPT_E_LIMIT, "acceleration structure too deep: a traversal could need " + std::to_string(need) +
                                            " stack entries, the kernels hold " + std::to_string(trace_stack_capacity()));
    }
    c->host_scene_ready = true;
    c->tlas_dirty = false;
    note_ties(c);
    if (c->device < 0) return JPT_OK;  // host-only context: arrays stay on the host, nothing can be rendered
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    HIP_TRY(c, b.tri_geom.upload(c->ref.tri_geom, s));
    {
        std::vector<ShadeTri> st(c->ref.tri_data.size());
        for (size_t i = 0; i < st.size(); i++) {
            const RefTriData& t = c->ref.tri_data[i];
            ShadeTri& o = st[i];
            for (int k = 0; k < 3; k++) o.n0[k] = t.n0[k];
            o.n1[0] = t.n1.x; o.n1[1] = t.n1.y; o.n1[2] = t.n1.z;
            o.n2[0] = t.n2.x; o.n2[1] = t.n2.y; o.n2[2] = t.n2.z;
            for (int k = 0; k < 3; k++) o.uvs[k][0] = t.uvs[k][0], o.uvs[k][1] = t.uvs[k][1];
            o.material_index = t.material_index;
        }
        HIP_TRY(c, b.shade_tris.upload(st, s));
        HIP_TRY(c, hipStreamSynchronize(s));   // (the staging vector goes out of scope)
    }
    HIP_TRY(c, b.materials.upload(c->ref.materials, s));
    HIP_TRY(c, b.bvh.upload(c->ref.bvh_nodes, s));
    HIP_TRY(c, b.set[0].inst.upload(c->ref.instances, s));
    HIP_TRY(c, b.tlas.upload(c->ref.tlas_nodes, s));
    HIP_TRY(c, b.tex.upload(c->ref.textures, s));
    HIP_TRY(c, b.wblas.upload(c->wide.blas_nodes, s));
    HIP_TRY(c, b.wtlas.upload(c->wide.tlas_nodes, s));
    HIP_TRY(c, b.wtris.upload(c->wide.tris, s));
    HIP_TRY(c, b.winst.upload(c->wide.instances, s));
    HIP_TRY(c, b.set[0].winst4.upload(c->wide.instances4, s));
    HIP_TRY(c, b.reach_tri.upload(c->ref.reach_tri, s));
    HIP_TRY(c, b.set[0].reach.upload(c->ref.reach_inst, s));
    HIP_TRY(c, b.cut_boxes.upload(c->ref.inst_cut_boxes, s));
    HIP_TRY(c, b.cut_range.upload(c->ref.inst_cut_range, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const int rc = finish_upload(c, true);
    if (rc == JPT_OK) c->scene_ready = true;
    return rc;
}

// instances / TLAS of c->ref changed (BLASes did not): re-flatten that part and upload it
int upload_tlas_update(jpt_ctx* c)
{
    lights_stale(c, true);
    std::string err;
    const bool use4 = walks_nodes4(c);
    if (!reflatten_tlas(c->ref, c->wide, use4, err)) return fail(c, JPT_E_INVALID, "tlas update: " + err);
    const uint32_t need = use4 ? c->wide.stack_need4 : c->wide.stack_need2;
    if (need > trace_stack_capacity()) {
        c->scene_ready = c->host_scene_ready = false;
        return fail(c, JPT_E_LIMIT, "acceleration structure too deep after the TLAS update: a traversal could need " +
                                        std::to_string(need) + " stack entries, the kernels hold " + std::to_string(trace_stack_capacity()));
    }
    if (c->device < 0) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    // renders already queued on the stream still read the old records: let them finish before the buffers move
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, b.set[0].inst.upload(c->ref.instances, s));
    HIP_TRY(c, b.tlas.upload(c->ref.tlas_nodes, s));
    HIP_TRY(c, b.wtlas.upload(c->wide.tlas_nodes, s));
    HIP_TRY(c, b.winst.upload(c->wide.instances, s));
    HIP_TRY(c, b.set[0].winst4.upload(c->wide.instances4, s));
    HIP_TRY(c, b.set[0].reach.upload(c->ref.reach_inst, s));
    HIP_TRY(c, b.cut_boxes.upload(c->ref.inst_cut_boxes, s));
    HIP_TRY(c, b.cut_range.upload(c->ref.inst_cut_range, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return finish_upload(c, false);
}

int validate_ref_scene(jpt_ctx* c, const RefScene& r)
{
    if (r.tri_geom.size() != r.tri_data.size()) return fail(c, JPT_E_INVALID, "triangle geometry/data counts differ");
    if (r.materials.empty()) return fail(c, JPT_E_INVALID, "material table is empty (entry 0 is the default material)");
    for (const RefInstance& i : r.instances)
        if (i.blas_index >= r.bvh_nodes.size()) return fail(c, JPT_E_INVALID, "instance root index out of range");
    for (const RefBvhNode& n : r.bvh_nodes) {
        if (n.tri_count > 0) {
            if ((size_t)n.first_tri_index + n.tri_count > r.tri_geom.size())
                return fail(c, JPT_E_INVALID, "BVH leaf triangle range out of bounds");
        } else if (n.left_child >= r.bvh_nodes.size() || n.right_child >= r.bvh_nodes.size()) {
            return fail(c, JPT_E_INVALID, "BVH child index out of range");
        }
    }
    return JPT_OK;
}

}  // namespace

extern "C" {

int jpt_abi_version(void) { return JPT_ABI_VERSION; }

int jpt_create(int device_id, jpt_ctx** out)
{
    if (!out) return JPT_E_INVALID;
    *out = nullptr;
    if (device_id == JPT_DEVICE_HOST_ONLY) {  // builder-only context: no device is touched
        jpt_ctx* c = new (std::nothrow) jpt_ctx();
        if (!c) return JPT_E_DEVICE;
        c->device = -1;
        std::memset(&c->stats, 0, sizeof c->stats);
        std::memset(&c->camera, 0, sizeof c->camera);
        *out = c;
        return JPT_OK;
    }
    // (Six renders in flight want six hardware queues for their streams; the runtime makes GPU_MAX_HW_QUEUES per priority level, four
    // by default, and reads the variable at the process's first HIP call.  That is the HOST's to export before it starts threads --
    // jpt.h "Process environment"; the library never writes the environment, it only measures what it got: six_queues_probe.)
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return JPT_E_DEVICE;
    }
    if (device_id < 0 || device_id >= n) {
        g_create_error = "device id out of range";
        return JPT_E_INVALID;
    }
    jpt_ctx* c = new (std::nothrow) jpt_ctx();
    if (!c) return JPT_E_DEVICE;
    c->device = device_id;
    std::memset(&c->stats, 0, sizeof c->stats);
    std::memset(&c->camera, 0, sizeof c->camera);
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = c->pipe.create_events()) != hipSuccess) {
        g_create_error = std::string("HIP init: ") + hipGetErrorString(e);
        delete c;
        return JPT_E_DEVICE;
    }
    c->stream = c->own_stream;
    (void)tuning();  // environment switches are read here, once per process
    *out = c;
    return JPT_OK;
}

void jpt_destroy(jpt_ctx* c)
{
    if (!c) return;
    if (c->device < 0) {
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    c->image.destroy();
    c->primary.destroy();
    c->enc.destroy();
    c->upd.destroy_stream();
    c->pipe.destroy();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* jpt_last_error(const jpt_ctx* c) { return c ? c->error.c_str() : g_create_error.c_str(); }

int jpt_set_stream(jpt_ctx* c, void* hip_stream)
{
    if (!c || c->device < 0) return JPT_E_INVALID;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (next != c->stream) {
        // everything this context has queued is ordered by the old stream (uploads, accumulation kernels, the
        // events its helper streams wait on): drain it before work starts appearing on another one
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->pipe.workspaces_touched();
        c->stream = next;
    }
    return JPT_OK;
}

int jpt_get_stream(jpt_ctx* c, void** hip_stream)
{
    if (!c || !hip_stream) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no stream");
    *hip_stream = (void*)c->stream;
    return JPT_OK;
}

int jpt_scene_upload_reference_layout(jpt_ctx* c, const void* tri_geometry, uint32_t n_triangles, const void* tri_data,
                                      const void* materials, uint32_t n_materials, const void* bvh_nodes, uint32_t n_bvh_nodes,
                                      const void* blas_instances, uint32_t n_instances, const void* tlas_nodes,
                                      uint32_t n_tlas_nodes, const uint8_t* tex_rgba8, int32_t tex_res, int32_t n_layers)
{
    if (!c) return JPT_E_INVALID;
    if ((n_triangles && (!tri_geometry || !tri_data)) || (n_materials && !materials) || (n_bvh_nodes && !bvh_nodes) ||
        (n_instances && !blas_instances) || (n_tlas_nodes && !tlas_nodes))
        return fail(c, JPT_E_INVALID, "null buffer with non-zero count");
    if (n_tlas_nodes > 65536) return fail(c, JPT_E_LIMIT, "TLAS has more nodes than 16-bit child indices address (bvh.h:59)");
    if (n_instances > 32767) return fail(c, JPT_E_LIMIT, "more instances than a TLAS with 16-bit child indices can hold (bvh.h:59; 32 767)");
    const auto t0 = std::chrono::steady_clock::now();
    c->scene_ready = c->host_scene_ready = false;
    c->from_commit = false;
    drop_mesh_rigs(c);   // the scene they were set for is gone from here on, whether or not this upload is accepted
    c->upload_note.clear();
    RefScene up;
    auto put = [](auto& vec, const void* src, uint32_t n) {
        using T = typename std::remove_reference<decltype(vec)>::type::value_type;
        vec.resize(n);
        if (n) std::memcpy(vec.data(), src, (size_t)n * sizeof(T));
    };
    put(up.tri_geom, tri_geometry, n_triangles);
    put(up.tri_data, tri_data, n_triangles);
    put(up.materials, materials, n_materials);
    put(up.bvh_nodes, bvh_nodes, n_bvh_nodes);
    put(up.instances, blas_instances, n_instances);
    put(up.tlas_nodes, tlas_nodes, n_tlas_nodes);
    if (tex_rgba8 && tex_res > 0 && n_layers > 0) {
        up.textures.assign(tex_rgba8, tex_rgba8 + (size_t)tex_res * tex_res * 4 * n_layers);
        up.tex_res = tex_res;
        up.n_layers = n_layers;
    }
    int rc = validate_ref_scene(c, up);
    if (rc != JPT_OK) return rc;
    // Default: the kernels walk the NATIVE tree (four-child quantised records over the uploaded triangles) and the boxes of
    // the uploaded leaves / TLAS leaves become the reach records that keep the image the reference's (jpt_builder.h,
    // native_from_uploaded) -- the addon keeps GeometryGroup3D::build() and gets the fast route's rate.  Arrays the reach
    // rule does not apply to, JPT_UPLOAD_WALK_AS_GIVEN and JPT_UPLOAD_WALK=given are walked node for node as uploaded.
    bool native = c->upload_mode == JPT_UPLOAD_NATIVE_TREE && !tuning().upload_as_given;
    if (native) {
        std::string why;
        native = native_from_uploaded(up, c->ref, why);
        if (!native) c->upload_note = "reference-layout upload is walked as given: " + why;
    } else {
        c->upload_note = "reference-layout upload is walked as given: requested";
    }
    if (!native) {
        c->ref.clear();
        c->ref.tri_geom = std::move(up.tri_geom);
        c->ref.tri_data = std::move(up.tri_data);
        c->ref.materials = std::move(up.materials);
        c->ref.bvh_nodes = std::move(up.bvh_nodes);
        c->ref.instances = std::move(up.instances);
        c->ref.tlas_nodes = std::move(up.tlas_nodes);
        c->ref.textures = std::move(up.textures);
        c->ref.tex_res = up.tex_res;
        c->ref.n_layers = up.n_layers;
    }
    c->tree = native ? JPT_TREE_NATIVE_REACH : JPT_TREE_AS_GIVEN;
    rc = upload_scene(c);
    c->stats.last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int jpt_set_upload_mode(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_UPLOAD_NATIVE_TREE && mode != JPT_UPLOAD_WALK_AS_GIVEN) return fail(c, JPT_E_INVALID, "unknown upload mode");
    c->upload_mode = mode;
    return JPT_OK;
}

int jpt_scene_tree_kind(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (!c->host_scene_ready) return JPT_TREE_NONE;
    return c->tree;
}

const char* jpt_scene_upload_note(const jpt_ctx* c) { return c ? c->upload_note.c_str() : ""; }

int jpt_scene_ties_exact(jpt_ctx* c, const char** why_out)
{
    if (why_out) *why_out = "";
    if (!c) return JPT_E_INVALID;
    if (!c->host_scene_ready) return fail(c, JPT_E_STATE, "no scene");
    if (why_out) *why_out = c->ties_note.c_str();
    return c->ties_note.empty() ? 1 : 0;
}

int jpt_scene_begin(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    drop_mesh_rigs(c);
    c->builder.begin();
    c->pending_materials.clear();
    c->pending_tex.clear();
    c->pending_tex_res = c->pending_layers = 0;
    c->building = true;
    return JPT_OK;
}

int jpt_scene_add_mesh(jpt_ctx* c, const jpt_surface* surfaces, int32_t n_surfaces, uint32_t* mesh_id_out)
{
    if (!c || !c->building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (n_surfaces < 0 || (n_surfaces && !surfaces)) return fail(c, JPT_E_INVALID, "bad surface array");
    std::vector<SurfaceView> sv((size_t)n_surfaces);
    for (int32_t i = 0; i < n_surfaces; i++) {
        const jpt_surface& s = surfaces[i];
        if (s.n_indices < 0 || s.n_vertices < 0 || (s.n_indices && (!s.indices || !s.vertices || !s.normals || !s.uvs)))
            return fail(c, JPT_E_INVALID, "surface needs vertex, normal, uv and index arrays (bvh.cpp:195-198)");
        if (s.n_indices % 3) return fail(c, JPT_E_INVALID, "index count is not a multiple of 3");
        for (int32_t k = 0; k < s.n_indices; k++)
            if (s.indices[k] < 0 || s.indices[k] >= s.n_vertices) return fail(c, JPT_E_INVALID, "vertex index out of range");
        sv[i] = SurfaceView{s.vertices, s.normals, s.uvs, s.indices, s.n_vertices, s.n_indices};
    }
    const uint32_t id = c->builder.add_mesh(sv.data(), n_surfaces);
    if (mesh_id_out) *mesh_id_out = id;
    return JPT_OK;
}

int jpt_scene_add_instance(jpt_ctx* c, uint32_t mesh_id, const float* transform12, const int32_t* material_ids, int32_t n_ids)
{
    if (!c || !c->building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (!transform12 || n_ids < 0 || (n_ids && !material_ids)) return fail(c, JPT_E_INVALID, "bad instance arguments");
    if (!c->builder.add_instance(mesh_id, transform12, material_ids, n_ids)) return fail(c, JPT_E_INVALID, "unknown mesh id");
    return JPT_OK;
}

int jpt_scene_set_materials(jpt_ctx* c, const void* materials, uint32_t n_materials)
{
    if (!c || !c->building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (n_materials && !materials) return fail(c, JPT_E_INVALID, "null materials");
    c->pending_materials.resize(n_materials);
    if (n_materials) std::memcpy(c->pending_materials.data(), materials, (size_t)n_materials * sizeof(RefMaterial));
    return JPT_OK;
}

int jpt_scene_set_textures(jpt_ctx* c, const uint8_t* tex, int32_t tex_res, int32_t n_layers)
{
    if (!c || !c->building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    c->pending_tex.clear();
    c->pending_tex_res = c->pending_layers = 0;
    if (tex && tex_res > 0 && n_layers > 0) {
        c->pending_tex.assign(tex, tex + (size_t)tex_res * tex_res * 4 * n_layers);
        c->pending_tex_res = tex_res;
        c->pending_layers = n_layers;
    }
    return JPT_OK;
}

int jpt_scene_commit(jpt_ctx* c, int32_t builder)
{
    if (!c || !c->building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (builder != JPT_BUILD_REFERENCE_EXACT && builder != JPT_BUILD_SAH && builder != JPT_BUILD_SAH_WATERTIGHT)
        return fail(c, JPT_E_INVALID, "unknown builder");
    const BuildMode mode = builder == JPT_BUILD_SAH ? BuildMode::Sah : (builder == JPT_BUILD_SAH_WATERTIGHT ? BuildMode::SahWatertight : BuildMode::ReferenceExact);
    const auto t0 = std::chrono::steady_clock::now();
    c->scene_ready = c->host_scene_ready = false;
    drop_mesh_rigs(c);
    std::string err;
    if (!c->builder.commit(mode, c->ref, err))
        return fail(c, JPT_E_LIMIT, err);
    c->ref.materials = c->pending_materials;
    c->ref.textures = c->pending_tex;
    c->ref.tex_res = c->pending_tex_res;
    c->ref.n_layers = c->pending_layers;
    c->tree = builder == JPT_BUILD_SAH ? JPT_TREE_NATIVE_REACH : (builder == JPT_BUILD_SAH_WATERTIGHT ? JPT_TREE_NATIVE_WATERTIGHT : JPT_TREE_REFERENCE_EXACT);
    int rc = validate_ref_scene(c, c->ref);
    if (rc != JPT_OK) return rc;
    c->from_commit = true;
    c->upload_note.clear();
    rc = upload_scene(c);
    c->building = false;
    c->stats.last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int jpt_scene_share(jpt_ctx* dst, jpt_ctx* src)
{
    if (!dst || !src) return JPT_E_INVALID;
    if (dst == src) return JPT_OK;
    if (!src->host_scene_ready || src->building) return fail(dst, JPT_E_STATE, "the source context holds no committed scene");
    if (src->upd.mesh_deformed)
        return fail(dst, JPT_E_STATE, "the source context's meshes were deformed on the device (jpt_scene_update_mesh): its host copy of the scene is stale until the next jpt_scene_commit");
    if (src->from_commit && (src->tlas_dirty || src->upd.refit_active)) {  // bring the source's host arrays up to date with its last transforms
        const int rc = jpt_scene_update_tlas(src);
        if (rc != JPT_OK) return fail(dst, rc, std::string("source context: ") + src->error);
    }
    const auto t0 = std::chrono::steady_clock::now();
    dst->scene_ready = dst->host_scene_ready = false;
    drop_mesh_rigs(dst);
    dst->builder = src->builder;   // so that jpt_scene_set_instance_transform / update_tlas keep working on the copy
    dst->ref = src->ref;
    dst->tree = src->tree;
    dst->from_commit = src->from_commit;
    dst->upload_note = src->upload_note;
    dst->ties_note = src->ties_note;
    dst->building = false;
    const int rc = upload_scene(dst);   // flatten + upload to dst's device; no builder runs
    dst->stats.last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int jpt_scene_set_instance_transform(jpt_ctx* c, uint32_t instance, const float* transform12)
{
    if (const int rc = needs_scene(c, kFromCommit, "jpt_scene_set_instance_transform", " needs a scene made by jpt_scene_commit"); rc != JPT_OK) return rc;
    if (!transform12) return fail(c, JPT_E_INVALID, "null transform");
    if (!c->builder.set_instance_transform(instance, transform12)) return fail(c, JPT_E_INVALID, "no such instance");
    c->tlas_dirty = true;
    return JPT_OK;
}

int jpt_scene_update_tlas(jpt_ctx* c)
{
    if (const int rc = needs_scene(c, kFromCommit, "jpt_scene_update_tlas", " needs a scene made by jpt_scene_commit"); rc != JPT_OK) return rc;
    if (c->upd.mesh_deformed)
        return fail(c, JPT_E_STATE, "a mesh was deformed on the device (jpt_scene_update_mesh): the host's copy of the scene is stale until the next jpt_scene_commit");
    if (!c->tlas_dirty) return JPT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    if (!c->builder.rebuild_instances(build_mode(c), c->ref, err)) {
        c->scene_ready = c->host_scene_ready = false;
        return fail(c, JPT_E_LIMIT, err);
    }
    const int rc = upload_tlas_update(c);
    if (rc == JPT_OK) c->tlas_dirty = false;
    c->stats.last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int jpt_scene_update_reference_tlas(jpt_ctx* c, const void* blas_instances, uint32_t n_instances, const void* tlas_nodes,
                                    uint32_t n_tlas_nodes)
{
    if (!c) return JPT_E_INVALID;
    if (!c->host_scene_ready || c->building) return fail(c, JPT_E_STATE, "no scene to update");
    if ((n_instances && !blas_instances) || (n_tlas_nodes && !tlas_nodes)) return fail(c, JPT_E_INVALID, "null buffer with non-zero count");
    if (n_tlas_nodes > 65536) return fail(c, JPT_E_LIMIT, "TLAS has more nodes than 16-bit child indices address (bvh.h:59)");
    if (c->from_commit) return fail(c, JPT_E_STATE, "the scene was made by jpt_scene_commit: use jpt_scene_set_instance_transform / jpt_scene_update_tlas");
    if (n_instances != c->ref.instances.size())
        return fail(c, JPT_E_INVALID, "instance count changed: upload the whole scene again");
    const bool native = walks_nodes4(c);  // the upload built the native tree: instances are matched by the roots the caller named then
    const RefInstance* in = static_cast<const RefInstance*>(blas_instances);
    for (uint32_t i = 0; i < n_instances; i++) {
        RefInstance one;
        std::memcpy(&one, reinterpret_cast<const char*>(in) + (size_t)i * sizeof(RefInstance), sizeof one);
        if (one.blas_index != (native ? c->ref.up_blas_index[i] : c->ref.instances[i].blas_index))
            return fail(c, JPT_E_INVALID, "an instance now names another BLAS: upload the whole scene again");
    }
    const auto t0 = std::chrono::steady_clock::now();
    // keep the old arrays until the new ones are known to flatten
    std::vector<RefInstance> old_inst = c->ref.instances;
    std::vector<RefTlasNode> old_tlas = c->ref.tlas_nodes;
    std::vector<ReachInst> old_reach = c->ref.reach_inst;
    // ... and the shadow's instance level with them (native_instances_from_uploaded rewrites it): after a
    // rejected update exact ties must still be decided on the TLAS of the scene that is rendered
    std::vector<RefInstance> old_x_inst;
    std::vector<RefTlasNode> old_x_tlas;
    std::vector<uint32_t> old_up_index;
    if (native) {
        old_x_inst = c->ref.exact.instances;
        old_x_tlas = c->ref.exact.tlas_nodes;
        old_up_index = c->ref.up_blas_index;
    }
    if (native) {
        std::vector<RefInstance> ni(n_instances);
        std::vector<RefTlasNode> nt(n_tlas_nodes);
        if (n_instances) std::memcpy(ni.data(), blas_instances, (size_t)n_instances * sizeof(RefInstance));
        if (n_tlas_nodes) std::memcpy(nt.data(), tlas_nodes, (size_t)n_tlas_nodes * sizeof(RefTlasNode));
        std::string why;
        if (!native_instances_from_uploaded(ni, nt, c->ref, why))  // (c->ref is untouched when this fails)
            return fail(c, JPT_E_INVALID, "the new instance level does not fit the native tree of the last upload (" + why +
                                              "): upload the whole scene again, or with JPT_UPLOAD_WALK_AS_GIVEN");
    } else {
        if (n_instances) std::memcpy(c->ref.instances.data(), blas_instances, (size_t)n_instances * sizeof(RefInstance));
        c->ref.tlas_nodes.resize(n_tlas_nodes);
        if (n_tlas_nodes) std::memcpy(c->ref.tlas_nodes.data(), tlas_nodes, (size_t)n_tlas_nodes * sizeof(RefTlasNode));
    }
    int rc = upload_tlas_update(c);
    if (rc != JPT_OK && rc != JPT_E_DEVICE) {
        const std::string msg = c->error;
        c->ref.instances = old_inst;
        c->ref.tlas_nodes = old_tlas;
        c->ref.reach_inst = old_reach;
        if (native) {
            c->ref.exact.instances = old_x_inst;
            c->ref.exact.tlas_nodes = old_x_tlas;
            c->ref.up_blas_index = old_up_index;
            if (c->ref.exact.valid) c->ref.exact.finish(c->ref.triangles.size());
        }
        const int back = upload_tlas_update(c);
        c->host_scene_ready = (back == JPT_OK);
        c->scene_ready = c->host_scene_ready && c->device >= 0;
        c->error = msg;
    }
    c->stats.last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int jpt_scene_get_reference_buffer(jpt_ctx* c, int32_t which, void* out, size_t capacity, size_t* size_out)
{
    if (!c) return JPT_E_INVALID;
    if (c->upd.mesh_deformed)
        return fail(c, JPT_E_STATE, "a mesh was deformed on the device (jpt_scene_update_mesh): the host's copy of the scene is stale until the next jpt_scene_commit");
    if (c->upd.refit_active && (which == JPT_BUF_INSTANCES || which == JPT_BUF_TLAS_NODES || which == JPT_BUF_REACH_INSTANCES)) {
        // the instance level was last refitted on the device: bring the host mirrors (and the device) to a fresh build
        const int rc = jpt_scene_update_tlas(c);
        if (rc != JPT_OK) return rc;
    }
    const void* src = nullptr;
    size_t bytes = 0;
    const RefScene& r = c->ref;
    switch (which) {
        case JPT_BUF_TRI_GEOMETRY: src = r.tri_geom.data(); bytes = r.tri_geom.size() * sizeof(RefTriGeometry); break;
        case JPT_BUF_TRI_DATA: src = r.tri_data.data(); bytes = r.tri_data.size() * sizeof(RefTriData); break;
        case JPT_BUF_MATERIALS: src = r.materials.data(); bytes = r.materials.size() * sizeof(RefMaterial); break;
        case JPT_BUF_BVH_NODES: src = r.bvh_nodes.data(); bytes = r.bvh_nodes.size() * sizeof(RefBvhNode); break;
        case JPT_BUF_INSTANCES: src = r.instances.data(); bytes = r.instances.size() * sizeof(RefInstance); break;
        case JPT_BUF_TLAS_NODES: src = r.tlas_nodes.data(); bytes = r.tlas_nodes.size() * sizeof(RefTlasNode); break;
        case JPT_BUF_TRIANGLES: src = r.triangles.data(); bytes = r.triangles.size() * sizeof(RefTriangle); break;
        case JPT_BUF_REACH_TRIANGLES: src = r.reach_tri.data(); bytes = r.reach_tri.size() * sizeof(ReachTri); break;
        case JPT_BUF_REACH_INSTANCES: src = r.reach_inst.data(); bytes = r.reach_inst.size() * sizeof(ReachInst); break;
        default: return fail(c, JPT_E_INVALID, "unknown buffer id");
    }
    if (size_out) *size_out = bytes;
    if (out) {
        if (capacity < bytes) return fail(c, JPT_E_INVALID, "buffer too small");
        if (bytes) std::memcpy(out, src, bytes);
    }
    return JPT_OK;
}

int jpt_set_camera(jpt_ctx* c, const void* camera160)
{
    if (!c || !camera160) return fail(c, JPT_E_INVALID, "null camera");
    std::memcpy(&c->camera, camera160, sizeof(RefCamera));
    c->camera_set = true;
    return JPT_OK;
}

int jpt_set_kernel(jpt_ctx* c, int32_t variant)
{
    if (!c) return JPT_E_INVALID;
    if (variant != JPT_KERNEL_WAVEFRONT && variant != JPT_KERNEL_REFERENCE_LAYOUT) return fail(c, JPT_E_INVALID, "unknown kernel variant");
    c->kernel_variant = variant;
    return JPT_OK;
}

int jpt_set_debug_steps(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    c->debug_steps = enable != 0;
    return JPT_OK;
}

int jpt_set_temporal_params(jpt_ctx* c, const void* render_parameters)
{
    if (!c) return JPT_E_INVALID;
    if (!render_parameters) return fail(c, JPT_E_INVALID, "null RenderParameters");
    std::memcpy(&c->reproj.temporal, render_parameters, sizeof(RefTemporalParams));
    c->reproj.temporal_set = true;
    return JPT_OK;
}

// ---- jpt_query_rays / jpt_query_pixels -----------------------------------------------------------------------------------------
// On the context's stream: behind the accumulation of every render queued so far and behind the device refits (queue_instance_refit
// makes the stream wait for each), and ahead of a later jpt_scene_update_mesh, whose drain event is recorded on this stream.  A
// later refit writes the copy of the instance level a query reads only after the event that retired it, recorded on this stream too.
constexpr uint32_t kQueryChunk = 1u << 20;   // rays per trip through the staging buffers (host forms)

// the checks every form shares, in the order the header gives: arguments, then the device, then the state; `done`: n == 0
static int query_checks(jpt_ctx* c, int32_t mode, const void* rays, uint32_t n, const void* hits, const void* occluded, const char* what, bool& done)
{
    done = false;
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_QUERY_CLOSEST && mode != JPT_QUERY_ANY) return fail(c, JPT_E_INVALID, std::string(what) + ": unknown mode");
    if (mode == JPT_QUERY_ANY && hits) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_ANY writes occluded_out only (hits_out must be NULL)");
    if (n == 0) {
        done = true;
        return JPT_OK;
    }
    if (!rays) return fail(c, JPT_E_INVALID, std::string(what) + ": null rays");
    if (mode == JPT_QUERY_CLOSEST && !hits) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_CLOSEST needs hits_out");
    if (mode == JPT_QUERY_ANY && !occluded) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_ANY needs occluded_out");
    return JPT_OK;
}

static int query_state(jpt_ctx* c, const char* what)
{
    if (c->device < 0) return fail(c, JPT_E_DEVICE, std::string("host-only context: ") + what + " runs on the device");
    if (!c->scene_ready) return fail(c, JPT_E_STATE, std::string(what) + ": no scene");
    HIP_TRY(c, hipSetDevice(c->device));
    return JPT_OK;
}

// One chunk of a host form: `m` rays (or, pixels: raster positions seen through that model) from `in` up, the walk, the results back into hits / occluded
// (either may be null).  Device layout of d_query: [rays 32 B][hits 64 B][bytes 1 B] per ray of a chunk, each part 16-byte aligned.
static int query_chunk(jpt_ctx* c, bool any, const CamModelDev* pixels, const void* in, uint32_t m, jpt_ray_hit* hits, uint8_t* occluded)
{
    const size_t cap = c->d_query.n / 97;
    char* d_rays = c->d_query.p;
    char* d_hits = d_rays + cap * sizeof(jpt_ray);
    char* d_occ = d_hits + cap * sizeof(jpt_ray_hit);
    char* h = c->image.h_read_pinned.as<char>();
    hipStream_t s = c->stream;
    if (pixels) {   // 8 B per ray go up, into the hits' part; the rays are made from them in place on the device
        std::memcpy(h, in, (size_t)m * 2 * sizeof(float));
        HIP_TRY(c, hipMemcpyAsync(d_hits, h, (size_t)m * 2 * sizeof(float), hipMemcpyHostToDevice, s));
        launch_query_pixel_rays(s, c->camera, *pixels, c->width, c->height, d_hits, m, d_rays);
    } else {
        std::memcpy(h, in, (size_t)m * sizeof(jpt_ray));
        HIP_TRY(c, hipMemcpyAsync(d_rays, h, (size_t)m * sizeof(jpt_ray), hipMemcpyHostToDevice, s));
    }
    launch_query(s, c->ds, any, d_rays, m, any ? nullptr : d_hits, occluded ? d_occ : nullptr);
    HIP_TRY(c, hipGetLastError());
    char* h_occ = h + (size_t)m * sizeof(jpt_ray_hit);
    if (hits) HIP_TRY(c, hipMemcpyAsync(h, d_hits, (size_t)m * sizeof(jpt_ray_hit), hipMemcpyDeviceToHost, s));
    if (occluded) HIP_TRY(c, hipMemcpyAsync(h_occ, d_occ, m, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (hits) std::memcpy(hits, h, (size_t)m * sizeof(jpt_ray_hit));
    if (occluded) std::memcpy(occluded, h_occ, m);
    return JPT_OK;
}

static int query_host(jpt_ctx* c, bool any, const CamModelDev* pixels, const void* in, uint32_t n, jpt_ray_hit* hits, uint8_t* occluded)
{
    const size_t cap = ((size_t)(n < kQueryChunk ? n : kQueryChunk) + 15) & ~(size_t)15;
    if (c->d_query.n < cap * 97) HIP_TRY(c, c->d_query.resize(cap * 97));
    HIP_TRY(c, c->image.h_read_pinned.reserve(cap * (sizeof(jpt_ray_hit) + 1)));
    const size_t in_stride = pixels ? 2 * sizeof(float) : sizeof(jpt_ray);
    for (size_t first = 0; first < n; first += kQueryChunk) {
        const uint32_t m = (uint32_t)(n - first < kQueryChunk ? n - first : kQueryChunk);
        const int rc = query_chunk(c, any, pixels, static_cast<const char*>(in) + first * in_stride, m, hits ? hits + first : nullptr,
                                   occluded ? occluded + first : nullptr);
        if (rc != JPT_OK) return rc;
    }
    return JPT_OK;
}

int jpt_query_rays(jpt_ctx* c, int32_t mode, const jpt_ray* rays, uint32_t n, jpt_ray_hit* hits_out, uint8_t* occluded_out)
{
    bool done;
    int rc = query_checks(c, mode, rays, n, hits_out, occluded_out, "jpt_query_rays", done);
    if (rc != JPT_OK || done) return rc;
    if ((rc = query_state(c, "jpt_query_rays")) != JPT_OK) return rc;
    return query_host(c, mode == JPT_QUERY_ANY, nullptr, rays, n, hits_out, occluded_out);
}

int jpt_query_rays_device(jpt_ctx* c, int32_t mode, const void* d_rays, uint32_t n, void* d_hits_out, void* d_occluded_out)
{
    bool done;
    int rc = query_checks(c, mode, d_rays, n, d_hits_out, d_occluded_out, "jpt_query_rays_device", done);
    if (rc != JPT_OK || done) return rc;
    const void* ptrs[3] = {d_rays, d_hits_out, d_occluded_out};
    for (const void* p : ptrs)
        if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) return fail(c, JPT_E_INVALID, "jpt_query_rays_device: the pointers must be 16-byte aligned");
    if ((rc = query_state(c, "jpt_query_rays_device")) != JPT_OK) return rc;
    for (const void* p : ptrs) {
        if (!p) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != c->device) {
            (void)hipGetLastError();
            return fail(c, JPT_E_INVALID, "jpt_query_rays_device: the pointers must be device memory of the context's device");
        }
    }
    launch_query(c->stream, c->ds, mode == JPT_QUERY_ANY, d_rays, n, d_hits_out, d_occluded_out);
    HIP_TRY(c, hipGetLastError());
    return JPT_OK;
}

int jpt_query_pixels(jpt_ctx* c, const float* xy, uint32_t n, jpt_ray_hit* hits_out)
{
    bool done;
    int rc = query_checks(c, JPT_QUERY_CLOSEST, xy, n, hits_out, nullptr, "jpt_query_pixels", done);
    if (rc != JPT_OK || done) return rc;
    if ((rc = query_state(c, "jpt_query_pixels")) != JPT_OK) return rc;
    if (!c->params_set || !c->camera_set) return fail(c, JPT_E_STATE, "jpt_query_pixels: jpt_set_params / jpt_set_camera not called");
    CamModelDev cm;   // (jpt_set_camera_model: picking follows the model)
    if ((rc = view_now(c, "jpt_query_pixels", "picking rays", cm)) != JPT_OK) return rc;
    return query_host(c, false, &cm, xy, n, hits_out, nullptr);
}

int jpt_get_stats(jpt_ctx* c, jpt_stats* out)
{
    if (!c || !out) return JPT_E_INVALID;
    *out = c->stats;
    return JPT_OK;
}

}  // extern "C"
