// jpt_scene.cpp -- the scene on the host (HostScene, jpt_ctx.h: the state table is at its declaration): the transitions and refusals its
// calls share, the uploads that bring it to the device (SceneBufs) and the view the kernels take of it, and the entry points that make,
// replace, move and read it -- jpt_scene_upload_reference_layout, jpt_set_upload_mode, jpt_scene_tree_kind, jpt_scene_upload_note,
// jpt_scene_ties_exact, jpt_scene_begin, jpt_scene_add_mesh, jpt_scene_add_instance, jpt_scene_set_materials, jpt_scene_set_textures,
// jpt_scene_commit, jpt_scene_share, jpt_scene_set_instance_transform, jpt_scene_update_tlas, jpt_scene_update_reference_tlas and
// jpt_scene_get_reference_buffer.  The calls that change a committed scene on the device are jpt_scene_update.cpp's.
#include "jpt_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "jpt_tuning.h"

// The view the kernels take (c->ds) of the scene's device arrays (c->dev): the counts from the host scene's ref / wide, the instance
// level the copy new renders read (cur_set).  Whether the tie shadow is usable and current (ds.x.ok, ds.x.tlas_current) is upload_shadow's.
void jpt::set_scene_view(jpt_ctx* c)
{
    const SceneBufs& b = c->dev;
    const SceneBufs::InstanceSet& is = b.set[c->upd.cur_set];
    const RefScene& r = c->scene.ref;
    const WideScene& w = c->scene.wide;
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
    d.use4 = c->scene.walks_nodes4();
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

// ---- the transitions and refusals more than one call shares ---------------------------------------------------------------------------

// The scene leaves the context: nothing answers for it from here on, and the rigs and regions set for it go with it
static void scene_left(jpt_ctx* c)
{
    c->scene.not_ready();
    drop_mesh_rigs(c);
}

// The one mapping between the builders of jpt_scene_commit, the tree kinds and the host builder's modes: the tree a builder makes
// (JPT_TREE_NONE: no such builder) ...
static int32_t tree_of_builder(int32_t build)
{
    switch (build) {
        case JPT_BUILD_REFERENCE_EXACT: return JPT_TREE_REFERENCE_EXACT;
        case JPT_BUILD_SAH: return JPT_TREE_NATIVE_REACH;
        case JPT_BUILD_SAH_WATERTIGHT: return JPT_TREE_NATIVE_WATERTIGHT;
        default: return JPT_TREE_NONE;
    }
}
// ... and the builder's mode for a tree (an as-given upload: ReferenceExact; rebuild_instances only sees committed scenes)
static BuildMode build_mode(int32_t tree)
{
    if (tree == JPT_TREE_NATIVE_REACH) return BuildMode::Sah;
    if (tree == JPT_TREE_NATIVE_WATERTIGHT) return BuildMode::SahWatertight;
    return BuildMode::ReferenceExact;
}

// the reference walks with two unchecked 64-entry stacks (main.glsl:272,307); here a deeper tree is an error when it is made
// instead of undefined behaviour at render time
int jpt::too_deep(jpt_ctx* c, uint32_t need, const char* after)
{
    return fail(c, JPT_E_LIMIT, std::string("acceleration structure too deep") + after + ": a traversal could need " + std::to_string(need) +
                                    " stack entries, the kernels hold " + std::to_string(trace_stack_capacity()));
}

static int host_copy_stale(jpt_ctx* c)
{
    return fail(c, JPT_E_STATE, "a mesh was deformed on the device (jpt_scene_update_mesh): the host's copy of the scene is stale until the next jpt_scene_commit");
}

int jpt::needs_scene(jpt_ctx* c, SceneNeed need, const char* call, const char* what, const char* exact, const char* sah)
{
    if (!c) return JPT_E_INVALID;
    const std::string own = std::string(call) + what;
    const HostScene& sc = c->scene;
    if (!sc.host_ready || sc.building || !sc.from_commit) return fail(c, JPT_E_STATE, own);
    if (need != kFromCommit && !sc.walks_nodes4()) return fail(c, JPT_E_STATE, exact ? exact : own);
    if (need == kWatertightTree && sc.tree != JPT_TREE_NATIVE_WATERTIGHT) return fail(c, JPT_E_STATE, sah ? sah : own);
    return JPT_OK;
}

int jpt::on_device(jpt_ctx* c, const char* host_only, bool scene)
{
    if (c->device < 0) return fail(c, JPT_E_DEVICE, host_only);
    if (scene && (!c->scene.device_ready || !c->ds.use4)) return fail(c, JPT_E_STATE, "no scene on the device");
    return JPT_OK;
}

namespace {

// ---- the uploads ----------------------------------------------------------------------------------------------------------------------

// Four-child records on the device: [ BLAS records | TLAS records ], internal child references of the TLAS part and
// the TLAS root shifted by the BLAS count.  The TLAS part has room for the largest TLAS of this instance count
// (<= one record per instance), so a TLAS update rewrites the tail only.
int upload_nodes4(jpt_ctx* c, bool tlas_only)
{
    const WideScene& w = c->scene.wide;
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
    HostScene& sc = c->scene;
    const ExactShadow& x = sc.ref.exact;
    sc.ties_note.clear();
    if (sc.walks_nodes4()) {
        if (sc.ref.reach_tri.empty()) sc.ties_note = "the scene has no reach records (JPT_BUILD_SAH_WATERTIGHT): the native tree's order decides";
        else if (x.instances.empty()) sc.ties_note.clear();   // nothing to hit
        else if (!x.valid) sc.ties_note = "the reference's TLAS of this scene could not be built (TLAS::build, bvh.cpp:264-317)";
        else if (!x.resolvable)
            sc.ties_note = "the uploaded trees are not in the shape the restricted walk indexes: every BLAS numbered in pre-order "
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
    const ExactShadow& x = c->scene.ref.exact;
    note_ties(c);
    if (!x.valid || !x.resolvable || !c->scene.walks_nodes4() || c->scene.ref.reach_tri.empty() || c->device < 0 || x.instances.empty())
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

// The instance level of the host scene -> copy 0 of the device's, queued on the context's stream: what both uploads share (the
// caller synchronises: the vectors are pageable host memory)
int upload_instance_level(jpt_ctx* c)
{
    const RefScene& r = c->scene.ref;
    const WideScene& w = c->scene.wide;
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    HIP_TRY(c, b.set[0].inst.upload(r.instances, s));
    HIP_TRY(c, b.tlas.upload(r.tlas_nodes, s));
    HIP_TRY(c, b.wtlas.upload(w.tlas_nodes, s));
    HIP_TRY(c, b.winst.upload(w.instances, s));
    HIP_TRY(c, b.set[0].winst4.upload(w.instances4, s));
    HIP_TRY(c, b.set[0].reach.upload(r.reach_inst, s));
    HIP_TRY(c, b.cut_boxes.upload(r.inst_cut_boxes, s));
    HIP_TRY(c, b.cut_range.upload(r.inst_cut_range, s));
    return JPT_OK;
}

// What both uploads end with on the device, of the `whole` scene or of its instance level: the one place that says a host upload
// happened (SceneUpdates::host_uploaded; a host-only context never leaves that state), then the four-child records, the shadow and the view
int finish_upload(jpt_ctx* c, bool whole)
{
    c->upd.host_uploaded(whole, c->scene.wide);
    int rc = upload_nodes4(c, !whole);
    if (rc != JPT_OK) return rc;
    rc = upload_shadow(c, !whole);
    set_scene_view(c);
    return rc;
}

// host RefScene (+ flatten) -> device
int upload_scene(jpt_ctx* c)
{
    HostScene& sc = c->scene;
    drop_mesh_rigs(c);   // (before anything can refuse the scene: no rig outlives the scene it was set for)
    lights_stale(c, true);
    std::string err;
    if (!flatten(sc.ref, sc.wide, err)) return fail(c, JPT_E_INVALID, "flatten: " + err);
    if (sc.walks_nodes4()) flatten4(sc.wide);
    else {
        sc.wide.blas_nodes4.clear();
        sc.wide.tlas_nodes4.clear();
        sc.wide.instances4.clear();
    }
    compute_stack_need(sc.wide);
    if (sc.stack_need() > trace_stack_capacity()) return too_deep(c, sc.stack_need(), "");
    sc.host_ready = true;
    sc.tlas_dirty = false;
    note_ties(c);
    if (c->device < 0) return JPT_OK;  // host-only context: arrays stay on the host, nothing can be rendered
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    HIP_TRY(c, b.tri_geom.upload(sc.ref.tri_geom, s));
    {
        std::vector<ShadeTri> st(sc.ref.tri_data.size());
        for (size_t i = 0; i < st.size(); i++) {
            const RefTriData& t = sc.ref.tri_data[i];
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
    HIP_TRY(c, b.materials.upload(sc.ref.materials, s));
    HIP_TRY(c, b.bvh.upload(sc.ref.bvh_nodes, s));
    HIP_TRY(c, b.tex.upload(sc.ref.textures, s));
    HIP_TRY(c, b.wblas.upload(sc.wide.blas_nodes, s));
    HIP_TRY(c, b.wtris.upload(sc.wide.tris, s));
    HIP_TRY(c, b.reach_tri.upload(sc.ref.reach_tri, s));
    if (const int rc = upload_instance_level(c); rc != JPT_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    const int rc = finish_upload(c, true);
    if (rc == JPT_OK) sc.device_ready = true;
    return rc;
}

// instances / TLAS of the host scene changed (BLASes did not): re-flatten that part and upload it
int upload_tlas_update(jpt_ctx* c)
{
    HostScene& sc = c->scene;
    lights_stale(c, true);
    std::string err;
    if (!reflatten_tlas(sc.ref, sc.wide, sc.walks_nodes4(), err)) return fail(c, JPT_E_INVALID, "tlas update: " + err);
    if (sc.stack_need() > trace_stack_capacity()) {
        sc.not_ready();
        return too_deep(c, sc.stack_need(), " after the TLAS update");
    }
    if (c->device < 0) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // renders already queued on the stream still read the old records: let them finish before the buffers move
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (const int rc = upload_instance_level(c); rc != JPT_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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

// The instance level of a scene, kept while jpt_scene_update_reference_tlas tries new arrays: they are only known to be good once
// they flatten.  It stops at the three vectors both routes restore.  The native route's own part (the shadow's instance level,
// up_blas_index and exact.finish) stays written out in the call: no test reaches a rollback of a native scene -- its new arrays are
// refused before they are taken, and no native TLAS made of them has come out too deep -- so that code is not moved.
struct InstanceLevelSnapshot {
    std::vector<RefInstance> instances;
    std::vector<RefTlasNode> tlas_nodes;
    std::vector<ReachInst> reach_inst;
    void save(const RefScene& r) { instances = r.instances, tlas_nodes = r.tlas_nodes, reach_inst = r.reach_inst; }
    void restore(RefScene& r) const { r.instances = instances, r.tlas_nodes = tlas_nodes, r.reach_inst = reach_inst; }
};

}  // namespace

extern "C" {

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
    HostScene& sc = c->scene;
    scene_left(c);   // the scene is gone from here on, whether or not this upload is accepted
    sc.from_commit = false;
    sc.upload_note.clear();
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
    bool native = sc.upload_mode == JPT_UPLOAD_NATIVE_TREE && !tuning().upload_as_given;
    if (native) {
        std::string why;
        native = native_from_uploaded(up, sc.ref, why);
        if (!native) sc.upload_note = "reference-layout upload is walked as given: " + why;
    } else {
        sc.upload_note = "reference-layout upload is walked as given: requested";
    }
    // as given: the uploaded arrays are the scene (what RefScene::clear() empties is empty in `up`, and what it keeps -- the materials, the
    // textures and their size -- is `up`'s either way)
    if (!native) sc.ref = std::move(up);
    sc.tree = native ? JPT_TREE_NATIVE_REACH : JPT_TREE_AS_GIVEN;
    rc = upload_scene(c);
    c->stats.last_build_ms = ms_since(t0);
    return rc;
}

int jpt_set_upload_mode(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_UPLOAD_NATIVE_TREE && mode != JPT_UPLOAD_WALK_AS_GIVEN) return fail(c, JPT_E_INVALID, "unknown upload mode");
    c->scene.upload_mode = mode;
    return JPT_OK;
}

int jpt_scene_tree_kind(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (!c->scene.host_ready) return JPT_TREE_NONE;
    return c->scene.tree;
}

const char* jpt_scene_upload_note(const jpt_ctx* c) { return c ? c->scene.upload_note.c_str() : ""; }

int jpt_scene_ties_exact(jpt_ctx* c, const char** why_out)
{
    if (why_out) *why_out = "";
    if (!c) return JPT_E_INVALID;
    if (!c->scene.host_ready) return fail(c, JPT_E_STATE, "no scene");
    if (why_out) *why_out = c->scene.ties_note.c_str();
    return c->scene.ties_note.empty() ? 1 : 0;
}

int jpt_scene_begin(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    HostScene& sc = c->scene;
    drop_mesh_rigs(c);
    sc.builder.begin();
    sc.pending_materials.clear();
    sc.pending_tex.clear();
    sc.pending_tex_res = sc.pending_layers = 0;
    sc.building = true;
    return JPT_OK;
}

int jpt_scene_add_mesh(jpt_ctx* c, const jpt_surface* surfaces, int32_t n_surfaces, uint32_t* mesh_id_out)
{
    if (!c || !c->scene.building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
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
    const uint32_t id = c->scene.builder.add_mesh(sv.data(), n_surfaces);
    if (mesh_id_out) *mesh_id_out = id;
    return JPT_OK;
}

int jpt_scene_add_instance(jpt_ctx* c, uint32_t mesh_id, const float* transform12, const int32_t* material_ids, int32_t n_ids)
{
    if (!c || !c->scene.building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (!transform12 || n_ids < 0 || (n_ids && !material_ids)) return fail(c, JPT_E_INVALID, "bad instance arguments");
    if (!c->scene.builder.add_instance(mesh_id, transform12, material_ids, n_ids)) return fail(c, JPT_E_INVALID, "unknown mesh id");
    return JPT_OK;
}

int jpt_scene_set_materials(jpt_ctx* c, const void* materials, uint32_t n_materials)
{
    if (!c || !c->scene.building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    if (n_materials && !materials) return fail(c, JPT_E_INVALID, "null materials");
    c->scene.pending_materials.resize(n_materials);
    if (n_materials) std::memcpy(c->scene.pending_materials.data(), materials, (size_t)n_materials * sizeof(RefMaterial));
    return JPT_OK;
}

int jpt_scene_set_textures(jpt_ctx* c, const uint8_t* tex, int32_t tex_res, int32_t n_layers)
{
    if (!c || !c->scene.building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    HostScene& sc = c->scene;
    sc.pending_tex.clear();
    sc.pending_tex_res = sc.pending_layers = 0;
    if (tex && tex_res > 0 && n_layers > 0) {
        sc.pending_tex.assign(tex, tex + (size_t)tex_res * tex_res * 4 * n_layers);
        sc.pending_tex_res = tex_res;
        sc.pending_layers = n_layers;
    }
    return JPT_OK;
}

int jpt_scene_commit(jpt_ctx* c, int32_t builder)
{
    if (!c || !c->scene.building) return fail(c, JPT_E_STATE, "jpt_scene_begin not called");
    const int32_t tree = tree_of_builder(builder);
    if (tree == JPT_TREE_NONE) return fail(c, JPT_E_INVALID, "unknown builder");
    const auto t0 = std::chrono::steady_clock::now();
    HostScene& sc = c->scene;
    scene_left(c);
    std::string err;
    if (!sc.builder.commit(build_mode(tree), sc.ref, err))
        return fail(c, JPT_E_LIMIT, err);
    sc.ref.materials = sc.pending_materials;
    sc.ref.textures = sc.pending_tex;
    sc.ref.tex_res = sc.pending_tex_res;
    sc.ref.n_layers = sc.pending_layers;
    sc.tree = tree;
    int rc = validate_ref_scene(c, sc.ref);
    if (rc != JPT_OK) return rc;
    sc.from_commit = true;
    sc.upload_note.clear();
    rc = upload_scene(c);
    sc.building = false;
    c->stats.last_build_ms = ms_since(t0);
    return rc;
}

int jpt_scene_share(jpt_ctx* dst, jpt_ctx* src)
{
    if (!dst || !src) return JPT_E_INVALID;
    if (dst == src) return JPT_OK;
    if (!src->scene.host_ready || src->scene.building) return fail(dst, JPT_E_STATE, "the source context holds no committed scene");
    if (src->upd.mesh_deformed)
        return fail(dst, JPT_E_STATE, "the source context's meshes were deformed on the device (jpt_scene_update_mesh): its host copy of the scene is stale until the next jpt_scene_commit");
    if (src->scene.from_commit && (src->scene.tlas_dirty || src->upd.refit_active)) {  // bring the source's host arrays up to date with its last transforms
        const int rc = jpt_scene_update_tlas(src);
        if (rc != JPT_OK) return fail(dst, rc, std::string("source context: ") + src->error);
    }
    const auto t0 = std::chrono::steady_clock::now();
    scene_left(dst);
    HostScene& to = dst->scene;
    const HostScene& from = src->scene;
    to.builder = from.builder;   // so that jpt_scene_set_instance_transform / update_tlas keep working on the copy
    to.ref = from.ref;
    to.tree = from.tree;
    to.from_commit = from.from_commit;
    to.upload_note = from.upload_note;
    to.ties_note = from.ties_note;
    to.building = false;
    const int rc = upload_scene(dst);   // flatten + upload to dst's device; no builder runs
    dst->stats.last_build_ms = ms_since(t0);
    return rc;
}

int jpt_scene_set_instance_transform(jpt_ctx* c, uint32_t instance, const float* transform12)
{
    if (const int rc = needs_scene(c, kFromCommit, "jpt_scene_set_instance_transform", " needs a scene made by jpt_scene_commit"); rc != JPT_OK) return rc;
    if (!transform12) return fail(c, JPT_E_INVALID, "null transform");
    if (!c->scene.builder.set_instance_transform(instance, transform12)) return fail(c, JPT_E_INVALID, "no such instance");
    c->scene.tlas_dirty = true;
    return JPT_OK;
}

int jpt_scene_update_tlas(jpt_ctx* c)
{
    if (const int rc = needs_scene(c, kFromCommit, "jpt_scene_update_tlas", " needs a scene made by jpt_scene_commit"); rc != JPT_OK) return rc;
    if (c->upd.mesh_deformed) return host_copy_stale(c);
    HostScene& sc = c->scene;
    if (!sc.tlas_dirty) return JPT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    if (!sc.builder.rebuild_instances(build_mode(sc.tree), sc.ref, err)) {
        sc.not_ready();
        return fail(c, JPT_E_LIMIT, err);
    }
    const int rc = upload_tlas_update(c);
    if (rc == JPT_OK) sc.tlas_dirty = false;
    c->stats.last_build_ms = ms_since(t0);
    return rc;
}

int jpt_scene_update_reference_tlas(jpt_ctx* c, const void* blas_instances, uint32_t n_instances, const void* tlas_nodes,
                                    uint32_t n_tlas_nodes)
{
    if (!c) return JPT_E_INVALID;
    HostScene& sc = c->scene;
    if (!sc.host_ready || sc.building) return fail(c, JPT_E_STATE, "no scene to update");
    if ((n_instances && !blas_instances) || (n_tlas_nodes && !tlas_nodes)) return fail(c, JPT_E_INVALID, "null buffer with non-zero count");
    if (n_tlas_nodes > 65536) return fail(c, JPT_E_LIMIT, "TLAS has more nodes than 16-bit child indices address (bvh.h:59)");
    if (sc.from_commit) return fail(c, JPT_E_STATE, "the scene was made by jpt_scene_commit: use jpt_scene_set_instance_transform / jpt_scene_update_tlas");
    RefScene& ref = sc.ref;
    if (n_instances != ref.instances.size())
        return fail(c, JPT_E_INVALID, "instance count changed: upload the whole scene again");
    const bool native = sc.walks_nodes4();  // the upload built the native tree: instances are matched by the roots the caller named then
    const RefInstance* in = static_cast<const RefInstance*>(blas_instances);
    for (uint32_t i = 0; i < n_instances; i++) {
        RefInstance one;
        std::memcpy(&one, reinterpret_cast<const char*>(in) + (size_t)i * sizeof(RefInstance), sizeof one);
        if (one.blas_index != (native ? ref.up_blas_index[i] : ref.instances[i].blas_index))
            return fail(c, JPT_E_INVALID, "an instance now names another BLAS: upload the whole scene again");
    }
    const auto t0 = std::chrono::steady_clock::now();
    // keep the old arrays until the new ones are known to flatten
    InstanceLevelSnapshot old;
    old.save(ref);
    // ... and the shadow's instance level with them (native_instances_from_uploaded rewrites it): after a
    // rejected update exact ties must still be decided on the TLAS of the scene that is rendered
    std::vector<RefInstance> old_x_inst;
    std::vector<RefTlasNode> old_x_tlas;
    std::vector<uint32_t> old_up_index;
    if (native) {
        old_x_inst = ref.exact.instances;
        old_x_tlas = ref.exact.tlas_nodes;
        old_up_index = ref.up_blas_index;
    }
    if (native) {
        std::vector<RefInstance> ni(n_instances);
        std::vector<RefTlasNode> nt(n_tlas_nodes);
        if (n_instances) std::memcpy(ni.data(), blas_instances, (size_t)n_instances * sizeof(RefInstance));
        if (n_tlas_nodes) std::memcpy(nt.data(), tlas_nodes, (size_t)n_tlas_nodes * sizeof(RefTlasNode));
        std::string why;
        if (!native_instances_from_uploaded(ni, nt, ref, why))  // (ref is untouched when this fails)
            return fail(c, JPT_E_INVALID, "the new instance level does not fit the native tree of the last upload (" + why +
                                              "): upload the whole scene again, or with JPT_UPLOAD_WALK_AS_GIVEN");
    } else {
        if (n_instances) std::memcpy(ref.instances.data(), blas_instances, (size_t)n_instances * sizeof(RefInstance));
        ref.tlas_nodes.resize(n_tlas_nodes);
        if (n_tlas_nodes) std::memcpy(ref.tlas_nodes.data(), tlas_nodes, (size_t)n_tlas_nodes * sizeof(RefTlasNode));
    }
    int rc = upload_tlas_update(c);
    if (rc != JPT_OK && rc != JPT_E_DEVICE) {
        const std::string msg = c->error;
        old.restore(ref);
        if (native) {
            ref.exact.instances = old_x_inst;
            ref.exact.tlas_nodes = old_x_tlas;
            ref.up_blas_index = old_up_index;
            if (ref.exact.valid) ref.exact.finish(ref.triangles.size());
        }
        const int back = upload_tlas_update(c);
        sc.host_ready = (back == JPT_OK);
        sc.device_ready = sc.host_ready && c->device >= 0;
        c->error = msg;
    }
    c->stats.last_build_ms = ms_since(t0);
    return rc;
}

int jpt_scene_get_reference_buffer(jpt_ctx* c, int32_t which, void* out, size_t capacity, size_t* size_out)
{
    if (!c) return JPT_E_INVALID;
    if (c->upd.mesh_deformed) return host_copy_stale(c);
    if (c->upd.refit_active && (which == JPT_BUF_INSTANCES || which == JPT_BUF_TLAS_NODES || which == JPT_BUF_REACH_INSTANCES)) {
        // the instance level was last refitted on the device: bring the host mirrors (and the device) to a fresh build
        const int rc = jpt_scene_update_tlas(c);
        if (rc != JPT_OK) return rc;
    }
    const void* src = nullptr;
    size_t bytes = 0;
    const RefScene& r = c->scene.ref;
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

}  // extern "C"
