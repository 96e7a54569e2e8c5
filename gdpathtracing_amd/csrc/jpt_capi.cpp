// jpt_capi.cpp -- the C ABI of include/jpt.h over the HIP kernels and the host builder.
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

int32_t rows_of_rank(int32_t height, int32_t rank, int32_t world)
{
    const int32_t n_strips = (height + kStripRows - 1) / kStripRows;
    int32_t rows = 0;
    for (int32_t s = rank; s < n_strips; s += world) {
        const int32_t y0 = s * kStripRows;
        rows += (y0 + kStripRows <= height) ? kStripRows : (height - y0);
    }
    return rows;
}

int32_t max_rows_of_any_rank(int32_t height, int32_t world)
{
    int32_t m = 0;
    for (int32_t r = 0; r < world; r++) m = std::max(m, rows_of_rank(height, r, world));
    return m;
}

// The blocking read-backs' pinned staging buffer grows to the largest read-back ever made (133 MB after one jpt_read_accum_f32 of a
// 3840 x 2160 image) and would otherwise be held until jpt_destroy: given back whenever the framebuffers are re-made (another
// resolution or partition) and by jpt_set_memory_policy; the next read-back allocates what it needs.
void release_read_staging(jpt_ctx* c) { c->h_read_pinned.release(); }

int alloc_framebuffers(jpt_ctx* c)
{
    if ((size_t)max_rows_of_any_rank(c->height, c->world) * c->width != c->d_accum.n) release_read_staging(c);
    c->local_rows = rows_of_rank(c->height, c->rank, c->world);
    // every rank allocates the same (maximum) size so a gather sees equal-sized pieces
    const size_t npx = (size_t)max_rows_of_any_rank(c->height, c->world) * c->width;
    HIP_TRY(c, c->d_accum.resize(npx));
    HIP_TRY(c, c->d_ldr.resize(npx));
    HIP_TRY(c, c->d_depth.resize(npx));
    HIP_TRY(c, c->d_counters.resize(1));
    if (npx) {
        HIP_TRY(c, hipMemsetAsync(c->d_accum.p, 0, npx * sizeof(float4), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_ldr.p, 0, npx * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_depth.p, 0, npx * sizeof(float), c->stream));
    }
    c->frame_count = 0;
    c->accum_restarts++;
    c->assembled = c->assembled_ldr = false;
    c->post.framebuffers_remade(false);
    return JPT_OK;
}

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

// Screen rectangles of the boxes the TLAS root offers (SkyCull, jpt_kernels.h).  A primary ray is the half-line from
// camera.position through ivp * (ndc, 1, 1) (main.glsl:411-420).  The projection used here is the double-precision
// inverse of that same ivp, and every projected corner is checked to lie on the ray of its own projection; if the
// camera block does not behave like a pinhole seen from `position` (inconsistent vp / ivp / position, a corner at or
// behind the camera), culling is off for this render.  Rectangles are widened by two pixels: the jitter stays inside
// the pixel (main.glsl:183-187) and float rounding of the ray set-up is orders of magnitude below a pixel.
void compute_sky_cull(const jpt_ctx* c, SkyCull& out)
{
    out.n = -1;
    if (!tuning().sky_cull || c->width <= 0 || c->height <= 0) return;
    if (!c->upd.cull_boxes_current) return;  // the root's boxes were last refitted on the device only: the host copy is stale
    // the boxes: children of the TLAS root record in the layout the kernels walk
    double lo[4][3], hi[4][3];
    int n = 0;
    const WideScene& w = c->wide;
    const bool use4 = walks_nodes4(c);
    if (w.instances.empty()) return;
    if (use4) {
        if (w.tlas_root4 < 0 || (size_t)w.tlas_root4 >= w.tlas_nodes4.size()) return;  // the root is a single instance
        const WideNode4& r = w.tlas_nodes4[(size_t)w.tlas_root4];
        for (int k = 0; k < 4; k++)
            if (r.child[k] != kEmptyChild) {
                lo[n][0] = r.lo_x[k]; lo[n][1] = r.lo_y[k]; lo[n][2] = r.lo_z[k];
                hi[n][0] = r.hi_x[k]; hi[n][1] = r.hi_y[k]; hi[n][2] = r.hi_z[k];
                n++;
            }
    } else {
        if (w.tlas_root < 0 || (size_t)w.tlas_root >= w.tlas_nodes.size()) return;
        const WideNode& r = w.tlas_nodes[(size_t)w.tlas_root];
        if (r.left == w.tlas_root && r.right == w.tlas_root) return;
        for (int k = 0; k < 3; k++) {
            lo[0][k] = r.lmin[k]; hi[0][k] = r.lmax[k];
            lo[1][k] = r.rmin[k]; hi[1][k] = r.rmax[k];
        }
        n = 2;
    }
    // vp' = inverse of ivp (column-major), in double
    double a[4][8];
    for (int r = 0; r < 4; r++)
        for (int col = 0; col < 4; col++) {
            a[r][col] = (double)c->camera.ivp[col * 4 + r];
            a[r][4 + col] = r == col ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; col++) {
        int piv = col;
        for (int r = col + 1; r < 4; r++)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (!(std::fabs(a[piv][col]) > 0.0) || !std::isfinite(a[piv][col])) return;
        if (piv != col)
            for (int k = 0; k < 8; k++) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 8; k++) a[col][k] /= d;
        for (int r = 0; r < 4; r++)
            if (r != col) {
                const double f = a[r][col];
                for (int k = 0; k < 8; k++) a[r][k] -= f * a[col][k];
            }
    }
    auto vp = [&](int r, int col) { return a[r][4 + col]; };
    const double O[3] = {(double)c->camera.position.x, (double)c->camera.position.y, (double)c->camera.position.z};
    const double W = (double)c->width, H = (double)c->height;
    for (int b = 0; b < n; b++) {
        double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
        for (int corner = 0; corner < 8; corner++) {
            const double C[3] = {(corner & 1) ? hi[b][0] : lo[b][0], (corner & 2) ? hi[b][1] : lo[b][1], (corner & 4) ? hi[b][2] : lo[b][2]};
            if (!std::isfinite(C[0]) || !std::isfinite(C[1]) || !std::isfinite(C[2])) return;
            double clip[4];
            for (int r = 0; r < 4; r++) clip[r] = vp(r, 0) * C[0] + vp(r, 1) * C[1] + vp(r, 2) * C[2] + vp(r, 3);
            if (!(std::fabs(clip[3]) > 1e-12)) return;
            const double nx = clip[0] / clip[3], ny = clip[1] / clip[3];
            if (!std::isfinite(nx) || !std::isfinite(ny) || std::fabs(nx) > 1e6 || std::fabs(ny) > 1e6) return;
            // the ray of that projection, as the kernel builds it: from O through F = ivp * (nx, ny, 1, 1) / w
            double F[4];
            for (int r = 0; r < 4; r++)
                F[r] = (double)c->camera.ivp[0 * 4 + r] * nx + (double)c->camera.ivp[1 * 4 + r] * ny + (double)c->camera.ivp[2 * 4 + r] +
                       (double)c->camera.ivp[3 * 4 + r];
            if (!(std::fabs(F[3]) > 1e-300)) return;
            const double D[3] = {F[0] / F[3] - O[0], F[1] / F[3] - O[1], F[2] / F[3] - O[2]};
            const double V[3] = {C[0] - O[0], C[1] - O[1], C[2] - O[2]};
            const double dd = D[0] * D[0] + D[1] * D[1] + D[2] * D[2], vv = V[0] * V[0] + V[1] * V[1] + V[2] * V[2];
            const double dv = D[0] * V[0] + D[1] * V[1] + D[2] * V[2];
            if (!(dd > 0.0) || !(vv > 0.0) || !(dv > 0.0)) return;  // corner at / behind the camera, or a degenerate ray
            // distance of the corner from that ray, relative to its distance from the camera
            const double cross2 = vv - dv * dv / dd;
            if (!(cross2 <= 1e-8 * vv)) return;  // the block is not a pinhole seen from `position`
            const double px = (nx + 1.0) * 0.5 * W, py = (1.0 - ny) * 0.5 * H;  // main.glsl:411-412 inverted
            x0 = std::min(x0, px); x1 = std::max(x1, px);
            y0 = std::min(y0, py); y1 = std::max(y1, py);
        }
        const double margin = 2.0;
        auto clampi = [](double v) { return (int32_t)std::max(-1.0e9, std::min(1.0e9, v)); };
        out.x0[b] = clampi(std::floor(x0 - margin));
        out.y0[b] = clampi(std::floor(y0 - margin));
        out.x1[b] = clampi(std::ceil(x1 + margin));
        out.y1[b] = clampi(std::ceil(y1 + margin));
    }
    for (int b = n; b < 4; b++) out.x0[b] = out.y0[b] = 1, out.x1[b] = out.y1[b] = 0;
    out.n = n;
}

int do_render_batch(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index, bool counted, bool blocking);

// frames of one wavefront render that fit the workspace budget (all frames of a batch are in flight at once)
int32_t frames_per_batch(const jpt_ctx* c, int32_t n_frames)
{
    const size_t budget = c->workspace_budget ? (size_t)c->workspace_budget : (size_t)tuning().workspace_budget_mb << 20;
    if (c->kernel_variant == JPT_KERNEL_REFERENCE_LAYOUT || c->debug_steps || n_frames <= 1) return n_frames;
    const size_t one = wf2_workspace_bytes(c->width, c->local_rows, 1, c->max_bounces, lighting_bound(c));
    const size_t fit = std::max<size_t>(1, budget / std::max<size_t>(one, 1));
    return (int32_t)std::min<size_t>((size_t)n_frames, fit);
}

// the statistics a blocking render in batches sums over its batches, f(a's field, b's field); the others are its last batch's
template <typename F>
void summed_stats(jpt_stats& a, const jpt_stats& b, F f)
{
    f(a.rays, b.rays);
    f(a.blas_expand, b.blas_expand);
    f(a.tri_tests, b.tri_tests);
    f(a.tlas_expand, b.tlas_expand);
    f(a.inst_visits, b.inst_visits);
    f(a.shaded_hits, b.shaded_hits);
    f(a.last_render_ms, b.last_render_ms);
    f(a.last_trace_ms, b.last_trace_ms);
    f(a.set_aside, b.set_aside);
    f(a.set_aside_dropped, b.set_aside_dropped);
}

int do_render(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index, bool counted, bool blocking)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0 || !c->scene_ready || !c->params_set || !c->camera_set || n_frames <= 0)
        return do_render_batch(c, n_frames, first_frame_index, counted, blocking);  // reports the error / no-op
    // a budget the caller set is a cap, not a hint: one frame is the smallest batch there is
    if (c->workspace_budget && c->kernel_variant != JPT_KERNEL_REFERENCE_LAYOUT && !c->debug_steps) {
        const size_t one = wf2_workspace_bytes(c->width, c->local_rows, 1, c->max_bounces, lighting_bound(c));
        if (one > c->workspace_budget)
            return fail(c, JPT_E_LIMIT, "jpt_set_memory_policy: one frame of this resolution needs a workspace of " + std::to_string(one) +
                                            " bytes, the budget is " + std::to_string(c->workspace_budget) +
                                            " (raise it, or render with JPT_KERNEL_REFERENCE_LAYOUT, which needs none)");
    }
    const int32_t per = frames_per_batch(c, n_frames);
    if (per >= n_frames) return do_render_batch(c, n_frames, first_frame_index, counted, blocking);
    // more frames than the workspace budget holds at once: batches in frame order (the accumulation continues).  A
    // queued render queues its batches (each takes the next pipeline slot; the statistics are those of the last one) ...
    if (!blocking && !counted) {
        for (int32_t done = 0; done < n_frames; done += per) {
            const int rc = do_render_batch(c, std::min(per, n_frames - done), first_frame_index + (uint32_t)done, false, false);
            if (rc != JPT_OK) return rc;
        }
        return JPT_OK;
    }
    // ... a blocking one runs them one after another, statistics summed over the batches
    jpt_stats sum;
    std::memset(&sum, 0, sizeof sum);
    for (int32_t done = 0; done < n_frames; done += per) {
        const int32_t nb = std::min(per, n_frames - done);
        const int rc = do_render_batch(c, nb, first_frame_index + (uint32_t)done, counted, true);
        if (rc != JPT_OK) return rc;
        summed_stats(sum, c->stats, [](auto& a, auto b) { a += b; });
    }
    summed_stats(c->stats, sum, [](auto& a, auto b) { a = b; });
    return JPT_OK;
}

// Helper streams and events are made on first use: most contexts (tests, tools, one-off renders) never queue renders
// or render enough paths to split them.  NOTE on hardware queues: the HIP runtime multiplexes the streams of a process
// onto GPU_MAX_HW_QUEUES hardware queues (default 4) per stream priority level, in the order of their first use, and two
// streams that share a queue execute in submission order.  With all of this library's streams at the normal level the
// rate of queued renders depended on which streams happened to share a queue (round 1, C3: 1.32 ms per render with the
// most fortunate order, 1.60 and 2.39 with others); the pipeline slots now take their queues from the highest priority
// level's pool (ensure_pipe_slot below), and so do the helper streams of frame groups (round 5: below).
bool ensure_pipe_slot(jpt_ctx* c, int k);
// frame groups: up to `groups - 1` helper streams (launch_wf2_render); returns how many there are, in order (0: one group)
int ensure_group_streams(jpt_ctx* c, int groups)
{
    Wf2Streams& gs = c->group_streams;
    if (!gs.fork && hipEventCreateWithFlags(&gs.fork, hipEventDisableTiming) != hipSuccess) {
        gs.fork = nullptr;
        (void)hipGetLastError();
        return 0;
    }
    int k = 0;
    for (; k + 1 < groups && k < kMaxGroups - 1; k++) {
        if (!gs.aux_stream[k]) {
            // The helper stream of group k + 1 IS pipeline slot k's stream (highest priority level by default, ensure_pipe_slot), not a
            // stream of its own at the context stream's level: the normal level's queues are dealt in the order of first use among ALL
            // the process's streams, and a helper that lands on the context stream's queue runs its group AFTER group 0 instead of
            // beside it -- 1.24 -> 1.48 ms per blocking C3 render after a counted render had run first, with six queues per level
            // (round 5, profiles/r05/r05an_...).  And not an extra stream at the slots' level either: a seventh stream there takes
            // one of the six queues the slots are measured to have to themselves (six_queues_probe).  A blocking render runs when
            // the renders queued before it have been ordered ahead of it on the context's stream; its groups queue behind whatever a
            // slot still holds.  (Normal / low slot priority chosen by the host: a stream of its own, as before.)
            const bool borrow = c->slot_priority != JPT_STREAM_PRIORITY_NORMAL && c->slot_priority != JPT_STREAM_PRIORITY_LOW;
            if (borrow) {
                if (!ensure_pipe_slot(c, k)) break;
                gs.aux_stream[k] = c->slot[k].stream;
                c->aux_borrowed[k] = true;
            } else if (hipStreamCreateWithFlags(&gs.aux_stream[k], hipStreamNonBlocking) != hipSuccess) {
                gs.aux_stream[k] = nullptr;
                (void)hipGetLastError();
                break;
            }
        }
        if (!gs.join[k] && hipEventCreateWithFlags(&gs.join[k], hipEventDisableTiming) != hipSuccess) {
            gs.join[k] = nullptr;
            (void)hipGetLastError();
            break;
        }
    }
    return k;
}
// render pipelining: stream + two events of slot k
bool ensure_pipe_slot(jpt_ctx* c, int k)
{
    PipeSlot& ps = c->slot[k];
    if (ps.stream && ps.ev_paths_done && ps.ev_acc_done) return true;
    bool ok = true;
    if (!ps.stream) {
        // Streams of different PRIORITY levels take their hardware queues from different pools (three levels on this
        // device, GPU_MAX_HW_QUEUES queues each).  The slots' four streams are created at the HIGHEST level: they have that
        // level's pool to themselves -- the host's streams, torch's, RCCL's and this library's own helper streams are all
        // at the normal level -- so they never share a queue, even when the pool is the runtime's default of four, which
        // a library cannot change (the variable is read at the process's first HIP call: tools/hwq_probe.py) and should not.
        // C3 queued rate in bench.py (torch loaded, counted and blocking renders before the timed region), pool of 4 / 16:
        // all slots normal 1.339 / 1.036 ms, all high 1.052 / 1.051, dealt over the three levels 1.230 / 1.212 (the normal-level
        // slot shares a queue with host streams), all low 1.137 / 1.135 (tools/prio_probe.sh, profiles/r02/prio_probe.txt).
        int least = 0, greatest = 0;
        // (the embedding application decides per context with jpt_set_stream_priority; the default is the highest level)
        const bool normal = c->slot_priority == JPT_STREAM_PRIORITY_NORMAL, low = c->slot_priority == JPT_STREAM_PRIORITY_LOW;
        if (!normal && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least > greatest)
            ok = hipStreamCreateWithPriority(&ps.stream, hipStreamNonBlocking, low ? least : greatest) == hipSuccess;
        else
            ok = hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking) == hipSuccess;
    }
    if (ok && !ps.ev_paths_done) ok = hipEventCreateWithFlags(&ps.ev_paths_done, hipEventDisableTiming) == hipSuccess;
    if (ok && !ps.ev_acc_done) ok = hipEventCreateWithFlags(&ps.ev_acc_done, hipEventDisableTiming) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// Do SIX of the slots' streams run side by side?  A stream runs on one of the hardware queues of its priority level's pool --
// GPU_MAX_HW_QUEUES per level, four by default, fixed at the process's first HIP call -- and streams that share a queue run one after
// the other: with the default pool a fifth and sixth render in flight cost 15-20 % (r04ad), with a pool of six or more they are worth
// 4 % on C3 and 15 % on small renders (profiles/r05/r05aj_slots_hw_queues_chain_sweep.txt).  The environment is the host's to set
// (bench.py and the Python binding do; jpt_create tries, jpt.h); what the library does is LOOK: one wave per slot stream busy for
// 0.4 ms, all six launched together -- side by side they are done in about that time, on four queues in about twice that.  Once per
// context, ~1 ms, before its first queued render.
bool six_queues_probe(jpt_ctx* c)
{
    if (c->six_queues >= 0) return c->six_queues != 0;
    c->six_queues = 0;
    constexpr int kProbe = 6;
    for (int k = 0; k < kProbe; k++)
        if (!ensure_pipe_slot(c, k)) return false;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        return false;
    }
    const long long ticks = (long long)khz * 400 / 1000;   // 0.4 ms
    for (int k = 0; k < kProbe; k++) launch_queue_spin(c->slot[k].stream, 1);   // (the module is loaded, the queues exist)
    for (int k = 0; k < kProbe; k++)
        if (hipStreamSynchronize(c->slot[k].stream) != hipSuccess) return false;
    double best = 1e9;
    for (int rep = 0; rep < 2; rep++) {   // the better of two: a host hiccup can only make it look serial
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < kProbe; k++) launch_queue_spin(c->slot[k].stream, ticks);
        for (int k = 0; k < kProbe; k++)
            if (hipStreamSynchronize(c->slot[k].stream) != hipSuccess) return false;
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    if (hipGetLastError() != hipSuccess) return false;
    c->six_queues = best < 0.4 * 1.6 ? 1 : 0;
    return c->six_queues != 0;
}

// the event the last render left on the context's stream has completed: nothing of this context is in flight
bool pipeline_idle(jpt_ctx* c)
{
    const bool idle = hipEventQuery(c->ev1) == hipSuccess;
    (void)hipGetLastError();   // (hipErrorNotReady is an answer, not an error)
    return idle;
}

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
const PlanDevice kPlanDevice{six_queues_probe, pipeline_idle, ensure_pipe_slot, ensure_group_streams};

// Every rule of a render's launch shape, in one place.  Makes no HIP call of its own; keeps c->last_pipe_slots and
// c->idle_streak.  fp: the render's frame_params; r: its sky cull and lighting.
LaunchPlan plan_launch(jpt_ctx* c, const FrameParams& fp, const Wf2Render& r, bool counted, bool blocking, const PlanDevice& dev)
{
    LaunchPlan p;
    if (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps) return p;   // (DEBUG_STEPS exists in the audit kernel only)
    const bool timed = c->kernel_timing;   // per-launch events want the launches of a render one after another
    // renders in flight (JPT_PIPE_SLOTS overrides): a render is eleven dependent launches of >= 25-30 us each
    // however little work it holds, so several of them are needed to fill the chip
    const int env_slots = tuning().pipe_slots;   // (after the embedding application's cap, jpt_set_memory_policy)
    const int forced_slots = c->max_slots > 0 ? c->max_slots : (env_slots <= 0 ? 0 : std::min(std::max(env_slots, 2), (int)jpt_ctx::kPipeSlots));
    // Four renders in flight, each tracing with a quarter of the blocks (four consecutive segments per block: a
    // deeper queue keeps a block's lanes refilled for a larger share of its launch) beat two renders of full-width
    // launches on every size tried: C3 1.32 vs 1.45 ms, C2 0.36 vs 0.46, 1 frame 0.30 vs 0.37, 1920x136 0.185 vs
    // 0.193, 4K x 16 spp 11.1 vs 11.1.  Renders whose workspace exceeds 24 GiB keep two slots and full-width launches
    // (4 x 24 GiB of workspaces is where this stops).
    const bool huge = wf2_workspace_bytes(c->width, c->local_rows, fp.n_frames, c->max_bounces, r.lighting) > ((size_t)24 << 30);
    // ... six where the slots' streams have six hardware queues to themselves (six_queues_probe), four otherwise
    const bool may_queue = tuning().pipelining && !blocking && !counted;
    const int slots = forced_slots ? forced_slots : (huge ? 2 : ((may_queue && dev.six_queues(c)) ? 6 : 4));
    if (may_queue) c->last_pipe_slots = slots;
    // A host that queues ONE render at a time (jpt_render_async, its own work, jpt_sync or the split read-back, again)
    // never has a second render in flight: the pipelined form's quarter-width launches then run alone, and a render takes
    // half as long again as a blocking one (C3 1.93 against 1.26 ms, 3840 x 2160 x 4 spp 3.33 against 2.11:
    // tools/lone_async_probe.py).  The third queued render in a row that finds nothing in flight -- the event every render
    // leaves on the context's stream has completed -- is launched like a blocking one instead (frame groups, full-width
    // launches; nobody waits for it here), and so on until a render finds work in flight.  A queue of renders is not
    // affected: only its first render finds the pipeline empty.
    bool lone = false;
    if (may_queue && !timed) {
        c->idle_streak = dev.idle(c) ? c->idle_streak + 1 : 0;
        lone = c->idle_streak >= 3;
    }
    const int slot = (int)(c->async_seq % (uint64_t)slots);
    if (may_queue && !timed && !lone && dev.slot_stream(c, slot)) {
        // (one frame group: overlapping with the neighbouring render does what groups do, without extra launches:
        // 3840x2160x16 spp 11.56 ms against 11.96 with two groups, instanced scene 3.80 against 4.05)
        p.route = LaunchPlan::kSlot;
        p.slot = slot;
        p.slots = slots;
        p.chain = (huge || slots == 1) ? 1 : 4;   // (a single render in flight: full-width launches)
        return p;
    }
    p.route = LaunchPlan::kStream;
    // Frame groups.  Every launch of the pipeline ends with a tail: a few long rays in a few waves while the rest of the
    // chip has nothing left to do (a ray's latency under full load is ~20 us on average, ~100 us for the longest; C3's ten
    // launch boundaries cost 0.5 ms of 1.85 -- render time is 0.48 + 0.17 * spp ms).  Balancing the queues does not
    // help (tried: equal ray counts per block, same time) and neither does fusing the bounce loop into one persistent
    // kernel (the barriers move into the blocks).  What helps is having other work ready when a launch drains: the
    // frames of a render are split into groups, each group runs the pipeline on its own stream with its own queues,
    // and the hardware fills the slots one group's kernel frees with the blocks of the other group's next kernel.
    // Measured on one MI355X (ms per blocking render, 1 / 2 / 3 / 4 groups of full-width launches): 3840x2160x16 spp 13.2 /
    // 11.9 / 12.2 / 13.1; 1920x1080x32 spp 5.92 / 5.38 / 5.75 / 6.18; x8 spp (C3) 1.81 / 1.80 / 2.09 / 2.54; x4 spp 1.17 /
    // 1.31: every extra launch costs ~25 us.  Two groups whose tracing launches are HALF as wide (two chained segments per
    // block, wf2_trace) do better, because the two groups' launches then really run side by side: C3 1.76 -> 1.61,
    // close-up 6.89 -> 6.22, 16 spp 3.11 -> 2.82, instanced scene 4.56 -> 4.03; 1280x720x4 spp 0.69 -> 0.71 (not used
    // below 12 M paths).  Counted and timed renders run in one group; so does one whose helper streams cannot be made.
    if (fp.n_frames >= 2 && !counted && !timed) {
        const int forced = std::min(std::max(tuning().groups, 0), kMaxGroups);   // JPT_GROUPS=n overrides the rule (tuning runs, tests)
        const size_t paths = (size_t)c->width * (size_t)c->local_rows * (size_t)fp.n_frames;
        const int wanted = std::min(fp.n_frames, forced ? forced : (paths >= ((size_t)12 << 20) ? 2 : 1));
        if (wanted > 1) p.groups = 1 + std::min(dev.group_streams(c, wanted), wanted - 1);
    }
    // Two frame groups share the chip: half-width launches.  A SMALL render that runs alone (the addon's use: one blocking
    // 1-spp frame per Godot frame): two chained segments per tracing block.  With a few rays per lane a segment's queue runs dry almost at once; half as
    // many waves with queues twice as deep keep their lanes fuller (C2 0.779 -> 0.738 ms, a 1-spp 1080p frame
    // 0.673 -> 0.648).  Not for windows of millions of paths (C3 in one group: 1.39 -> 1.51 ms) nor for scenes
    // past the caches, which are bound by the latency of their fetches and want every wave they can get (1 M
    // triangles, 2 spp: 9.49 -> 9.93 ms): one segment per block (profiles/r03/r03ao_lone_chain.txt).
    const uint64_t window_paths = ((uint64_t)c->width * (uint64_t)c->local_rows - wf2_pixels_outside_window(r.cull, fp)) * (uint64_t)fp.n_frames;
    const size_t walked_bytes = c->wide.blas_nodes4.size() * sizeof(WideNodeQ) + c->wide.tris.size() * sizeof(WideTri);
    const bool small = window_paths <= 1500000u && walked_bytes <= ((size_t)32 << 20);
    p.chain = (p.groups == 2 || (walks_nodes4(c) && small)) ? 2 : 1;
    return p;
}

// the frame parameters of a render of n_frames frames from first_frame_index
FrameParams frame_params(const jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index, bool want_depth)
{
    // (in the order of the fields: image, partition, bounces, accumulation, first frame, frames, depth frame, display, DEBUG_STEPS)
    return FrameParams{c->width, c->height, c->local_rows, c->rank, c->world, c->max_bounces, c->accum_mode, first_frame_index,
                       c->frame_count + 1, n_frames, want_depth ? n_frames - 1 : -1, c->denoise == JPT_DENOISE_PROGRESSIVE ? 0 : 1,
                       c->debug_steps ? 1 : 0};
}

// the sum of the kernel-timing event pairs of the last render; *primary_ms (unless null) gets the first pair's, wf2_primary's
double traced_ms(const jpt_ctx* c, double* primary_ms)
{
    double tms = 0.0;
    for (int32_t k = 0; k + 1 < c->trace_events_used; k += 2) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, c->trace_events[(size_t)k], c->trace_events[(size_t)k + 1]) == hipSuccess) {
            tms += t;
            if (k == 0 && primary_ms) *primary_ms = t;
        }
    }
    return tms;
}

int validate_render(jpt_ctx* c, int32_t n_frames)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context (JPT_DEVICE_HOST_ONLY) cannot render: there is no CPU fallback");
    if (!c->scene_ready) return fail(c, JPT_E_STATE, "no scene: call jpt_scene_upload_reference_layout or jpt_scene_commit first");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    if (!c->camera_set) return fail(c, JPT_E_STATE, "jpt_set_camera not called");
    if (n_frames < 0) return fail(c, JPT_E_INVALID, "n_frames < 0");
    if (c->upd.mesh_deformed && (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps))
        return fail(c, JPT_E_STATE, "jpt_scene_update_mesh refits the default kernel's records only: call jpt_scene_commit before rendering with another kernel");
    if (c->upd.refit_active && (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps))
        return fail(c, JPT_E_STATE, "jpt_scene_refit_tlas refits the default kernel's records only: call jpt_scene_update_tlas before rendering with another kernel");
    return JPT_OK;
}

// What a render needs before it is planned: the temporal pass's history, zeroed counters, the workspace of the context's
// stream, the timing events, and (wavefront renders) the sky cull and the tiles' sky cells in r.  r.lighting and r.primary are the render's.
int prepare_render(jpt_ctx* c, const FrameParams& fp, bool counted, bool wavefront, Wf2Render& r)
{
    hipStream_t s = c->stream;
    const int32_t n_frames = fp.n_frames;
    if (c->denoise == JPT_DENOISE_TEMPORAL) {
        // the pass runs once per displayed frame and reads other pixels' depth and history (temporal_reprojection.glsl:57-61)
        if (n_frames > 1) return fail(c, JPT_E_INVALID, "temporal reprojection renders one frame per call");
        if (c->world != 1) return fail(c, JPT_E_STATE, "temporal reprojection needs the whole image in one context (world == 1)");
        if (!c->temporal_set) return fail(c, JPT_E_STATE, "jpt_set_temporal_params not called");
        if (c->temporal.width != c->width || c->temporal.height != c->height)
            return fail(c, JPT_E_INVALID, "temporal RenderParameters width/height differ from jpt_set_params");
        const size_t npx = (size_t)c->width * c->height;
        if (!c->hist_valid || c->d_hist1.n != npx) {
            // Image::create(...) zero-filled history images (temporal_reprojection.cpp:42-43)
            HIP_TRY(c, hipStreamSynchronize(s));
            HIP_TRY(c, c->d_hist1.resize(npx));
            HIP_TRY(c, c->d_hist2.resize(npx));
            if (npx) {
                HIP_TRY(c, hipMemsetAsync(c->d_hist1.p, 0, npx * sizeof(float4), s));
                HIP_TRY(c, hipMemsetAsync(c->d_hist2.p, 0, npx * sizeof(float4), s));
            }
            c->hist_valid = true;
            c->hist_written = nullptr;
        }
    }
    if (counted) HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(DevCounters), s));
    const bool wf2 = wavefront && c->local_rows > 0 && c->width > 0 && n_frames > 0;
    if (wf2) {
        const size_t need = wf2_workspace_bytes(c->width, c->local_rows, n_frames, c->max_bounces, r.lighting);
        if (c->slot[0].workspace.n < need) {
            HIP_TRY(c, hipStreamSynchronize(s));
            HIP_TRY(c, c->slot[0].workspace.resize(need));
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev0, s));
    if (!wf2) return JPT_OK;
    const size_t need_ev = c->kernel_timing ? 2 * (size_t)(c->max_bounces + 1) : 0;
    while (c->trace_events.size() < need_ev) {
        hipEvent_t e;
        HIP_TRY(c, hipEventCreate(&e));
        c->trace_events.push_back(e);
    }
    c->trace_events_used = (int32_t)need_ev;
    if (!r.primary.sky_cull()) return JPT_OK;   // (r.cull stays off, n < 0, and r.sky_tiles null)
    if (r.variance) return JPT_OK;   // (likewise: jpt_set_variance's kernel reads every pixel's frames, and a culled pixel's are never stored)
    compute_sky_cull(c, r.cull);
    // the sky cells of whole tiles, for wf2_accumulate (REF_LDR8 sums of several frames): on the context's stream, which every
    // accumulation is ordered behind; again only when the camera (its frame index aside), the image size or the partition changed.
    // (With an environment map the accumulation makes up culled pixels exactly, frame by frame: the cells bound the gradient only.)
    if (c->accum_mode == JPT_ACCUM_REF_LDR8 && n_frames > 1 && r.lighting.env_mode == 0) {
        const int32_t key[5] = {c->width, c->height, c->local_rows, c->rank, c->world};
        RefCamera cam_key = c->camera;
        cam_key.frame_index = 0;
        const size_t n_tiles = wf2_sky_tile_count(c->width, c->local_rows);
        if (!c->sky_tiles_valid || c->d_sky_tiles.n < n_tiles || std::memcmp(key, c->sky_tiles_key, sizeof key) != 0 ||
            std::memcmp(&cam_key, &c->sky_tiles_camera, sizeof cam_key) != 0) {
            if (c->d_sky_tiles.n < n_tiles) {
                HIP_TRY(c, hipStreamSynchronize(s));   // (renders in flight may read the old buffer)
                for (const PipeSlot& ps : c->slot)
                    if (ps.stream) HIP_TRY(c, hipStreamSynchronize(ps.stream));
                HIP_TRY(c, c->d_sky_tiles.resize(n_tiles));
            }
            launch_sky_tiles(s, fp, c->camera, c->d_sky_tiles.p);
            std::memcpy(c->sky_tiles_key, key, sizeof key);
            c->sky_tiles_camera = cam_key;
            c->sky_tiles_valid = true;
        }
        r.sky_tiles = c->d_sky_tiles.p;
    }
    return JPT_OK;
}

// the render's launches on the route of its plan
int launch_render(jpt_ctx* c, const LaunchPlan& p, const FrameParams& fp, Wf2Render& r, DevCounters* cnt, float* depth_img)
{
    hipStream_t s = c->stream;
    if (p.route == LaunchPlan::kReference) {
        FrameParams one = fp;
        for (int32_t f = 0; f < fp.n_frames; f++) {
            one.frame_index = fp.frame_index + (uint32_t)f;
            one.frame_count = c->frame_count + (uint32_t)f + 1;
            one.n_frames = 1;
            one.depth_frame = 0;
            launch_ref_frame(s, c->ds, one, c->camera, c->d_accum.p, c->d_ldr.p, depth_img, cnt, r.lighting, r.primary);
        }
        return JPT_OK;
    }
    if (p.route == LaunchPlan::kStream) {
        launch_wf2_render(s, c->ds, fp, c->camera, c->slot[0].workspace.p, c->d_accum.p, c->d_ldr.p, depth_img, cnt,
                          c->kernel_timing ? c->trace_events.data() : nullptr, r, p.groups, p.chain, c->group_streams);
        return JPT_OK;
    }
    // a queued render: path kernels and accumulation on the slot's stream with the slot's workspace
    PipeSlot& ps = c->slot[p.slot];
    const size_t need = wf2_workspace_bytes(c->width, c->local_rows, fp.n_frames, c->max_bounces, r.lighting);
    bool slots_ready = true;
    for (int k = 0; k < p.slots; k++) slots_ready = slots_ready && c->slot[k].stream && c->slot[k].workspace.n >= need;
    if (!slots_ready) {
        // The first queued render of this size prepares ALL the slots, so that none of it lands in the middle
        // of a queue of renders: a stream that gets its own hardware queue costs ~6 ms to create, a device
        // allocation waits for the device, and a fresh 2 GB allocation costs its first user ~10 ms.
        HIP_TRY(c, hipStreamSynchronize(s));  // every earlier render ends with a kernel on `s`
        for (int k = 0; k < p.slots; k++) {
            PipeSlot& sk = c->slot[k];
            if (sk.workspace.n < need) {
                HIP_TRY(c, sk.workspace.resize(need));
                HIP_TRY(c, hipMemsetAsync(sk.workspace.p, 0, need, s));  // first touch
                sk.acc_done_valid = false;
            }
            if (!ensure_pipe_slot(c, k)) return fail(c, JPT_E_DEVICE, "cannot create the stream of a pipeline slot");
        }
    }
    // this workspace was last read by the accumulation of the render `slots` renders ago; when that is not on record
    // (first use of the slot, or renders that went through `s` itself since), wait for whatever `s` holds now
    if (!ps.acc_done_valid) HIP_TRY(c, hipEventRecord(ps.ev_acc_done, s));
    HIP_TRY(c, hipStreamWaitEvent(ps.stream, ps.ev_acc_done, 0));
    if (ps.refit_seen != c->upd.refit_wait_seq) {
        // the instance level this render reads was refitted on the refit stream (jpt_scene_refit_tlas)
        HIP_TRY(c, hipStreamWaitEvent(ps.stream, c->upd.ev_refit_done, 0));
        ps.refit_seen = c->upd.refit_wait_seq;
    }
    // The accumulation runs on the slot's stream too, after whatever `s` holds now (the previous render's accumulation, an
    // upload, a read-back), and `s` then waits for it: the results are those of serial execution, and `s` itself carries no
    // kernels of a render (the hardware runs a handful of queues side by side; a busy `s` would be one more)
    HIP_TRY(c, hipEventRecord(ps.ev_paths_done, s));
    r.before_acc = ps.ev_paths_done;
    launch_wf2_render(ps.stream, c->ds, fp, c->camera, ps.workspace.p, c->d_accum.p, c->d_ldr.p, depth_img, nullptr, nullptr, r,
                      p.groups, p.chain, c->group_streams);
    HIP_TRY(c, hipEventRecord(ps.ev_acc_done, ps.stream));
    HIP_TRY(c, hipStreamWaitEvent(s, ps.ev_acc_done, 0));
    ps.acc_done_valid = true;
    c->async_seq++;
    return JPT_OK;
}

// a blocking or counted render: its time, ray count and event counters
int read_back_stats(jpt_ctx* c, const FrameParams& fp, bool counted, bool wavefront, const SkyCull& cull)
{
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.last_render_ms = ms;
    c->stats.last_trace_ms = ms;
    if (wavefront && c->trace_events_used > 0 && fp.n_frames > 0 && c->local_rows > 0) c->stats.last_trace_ms = traced_ms(c, &c->stats.last_primary_ms);
    if (wavefront && c->slot[0].workspace.p && fp.n_frames > 0 && c->local_rows > 0) {
        // ray segments traced = sum of the per-bounce queue sizes (always available on this route)
        const size_t nq = (size_t)c->max_bounces + 2, per_row = wf2_segments();
        c->h_qcount.assign(nq * per_row + 2u, 0u);   // queue sizes, then the set-aside counts
        HIP_TRY(c, hipMemcpy(c->h_qcount.data(), c->slot[0].workspace.p, c->h_qcount.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        c->stats.set_aside = c->h_qcount[nq * per_row];
        c->stats.set_aside_dropped = c->h_qcount[nq * per_row + 1u];
        // every in-image (pixel, frame) has one primary segment; rows 1.. hold the later bounces' queue sizes
        uint64_t rays = (uint64_t)c->width * (uint64_t)c->local_rows * (uint64_t)fp.n_frames;
        for (int b = 1; b <= c->max_bounces; b++)
            for (size_t k = 0; k < per_row; k++) rays += c->h_qcount[(size_t)b * per_row + k];
        c->stats.rays = rays;
    }
    if (counted) {
        DevCounters h;
        HIP_TRY(c, hipMemcpy(&h, c->d_counters.p, sizeof h, hipMemcpyDeviceToHost));
        // (pixel, frame) pairs outside the render's window were never enumerated on the device: each is one primary
        // segment that ends at the TLAS root, like the culled ones inside the window
        const uint64_t outside = wavefront ? wf2_pixels_outside_window(cull, fp) * (uint64_t)fp.n_frames : 0;
        h.phase[7] += outside;
        c->stats.rays = h.rays + outside;
        c->stats.blas_expand = h.blas_expand;
        c->stats.tri_tests = h.tri_tests;
        c->stats.tlas_expand = h.tlas_expand + outside;
        c->stats.inst_visits = h.inst_visits;
        c->stats.shaded_hits = h.shaded_hits;
        for (int k = 0; k < 8; k++) c->stats.phase[k] = h.phase[k];
        c->stats.sky_culled = h.phase[7];
        c->stats.walk_steps_max = h.walk_max;
        for (int k = 0; k < 8; k++) c->stats.walk_steps_hist[k] = h.walk_hist[k];
        c->stats.zero_throughput = h.zero_thr;
    }
    return JPT_OK;
}

// validate -> prepare -> plan -> launch -> read back
int do_render_batch(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index, bool counted, bool blocking)
{
    int rc = validate_render(c, n_frames);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->assembled = c->assembled_ldr = false;
    const bool wavefront = c->kernel_variant == JPT_KERNEL_WAVEFRONT && !c->debug_steps;   // (DEBUG_STEPS exists in the audit kernel only)
    // the depth image (main.glsl:432,435) has one reader, the temporal pass: off when the host said so (jpt_set_outputs)
    const bool want_depth = (c->outputs & JPT_OUTPUT_DEPTH) != 0u || c->denoise == JPT_DENOISE_TEMPORAL;
    const FrameParams fp = frame_params(c, n_frames, first_frame_index, want_depth);
    Wf2Render r;
    if ((rc = check_bake_directional(c)) != JPT_OK) return rc;
    if ((rc = resolve_primary(c, r.primary)) != JPT_OK) return rc;
    if ((rc = resolve_lighting(c, r.lighting)) != JPT_OK) return rc;
    if (c->post.bake_dir && r.primary.kind == PrimaryRays::kBake && c->local_rows > 0 && n_frames > 0) {
        if ((rc = ensure_bake_dir(c)) != JPT_OK) return rc;
        r.bake_dir = c->post.d_bake_dir.p;
    }
    if ((rc = check_variance(c)) != JPT_OK) return rc;
    if (c->post.variance && c->local_rows > 0 && c->width > 0 && n_frames > 0) {
        if ((rc = ensure_variance(c)) != JPT_OK) return rc;
        r.variance = c->post.d_variance.p;
    }
    if ((rc = prepare_render(c, fp, counted, wavefront, r)) != JPT_OK) return rc;
    bool pipelined = false;
    if (c->local_rows > 0 && c->width > 0 && n_frames > 0) {
        c->depth_valid = want_depth;
        const LaunchPlan p = plan_launch(c, fp, r, counted, blocking, kPlanDevice);
        rc = launch_render(c, p, fp, r, counted ? c->d_counters.p : nullptr, want_depth ? c->d_depth.p : nullptr);
        if (rc != JPT_OK) return rc;
        if (r.bake_dir) c->post.bake_dir_valid = true;
        if (r.variance) c->post.variance_valid = true;
        pipelined = p.route == LaunchPlan::kSlot;
        if (c->denoise == JPT_DENOISE_TEMPORAL) {
            // TemporalReprojection::render's dispatch (temporal_reprojection.cpp:71): screen + depth of this frame in,
            // blended history and the displayed screen out
            launch_temporal(c->stream, c->temporal, c->d_ldr.p, c->d_depth.p, c->d_hist1.p, c->d_hist2.p);
            c->hist_written = (c->temporal.frame_count % 2u) == 0u ? c->d_hist2.p : c->d_hist1.p;
        }
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (wavefront && !pipelined) c->slot[0].acc_done_valid = false;  // slot 0's workspace was used on the context's stream itself
    c->frame_count += (uint32_t)n_frames;
    c->stats.frames = c->frame_count;
    return (blocking || counted) ? read_back_stats(c, fp, counted, wavefront, r.cull) : JPT_OK;
}

// local strip-major rows -> full image rows, on the host
template <typename T>
void scatter_rows(const T* local, T* out, int32_t width, int32_t height, int32_t rank, int32_t world, int comps)
{
    const int32_t n_strips = (height + kStripRows - 1) / kStripRows;
    int32_t ly = 0;
    for (int32_t s = rank; s < n_strips; s += world) {
        for (int32_t r = 0; r < kStripRows; r++) {
            const int32_t y = s * kStripRows + r;
            if (y >= height) break;
            std::memcpy(out + (size_t)y * width * comps, local + (size_t)ly * width * comps, (size_t)width * comps * sizeof(T));
            ly++;
        }
    }
}
template <typename T>
void scatter_rows(const std::vector<T>& local, T* out, int32_t width, int32_t height, int32_t rank, int32_t world, int comps)
{
    scatter_rows(local.data(), out, width, height, rank, world, comps);
}

// the pinned staging buffer of the display image's split read-backs (one full image)
int ensure_ldr_pinned(jpt_ctx* c)
{
    HIP_TRY(c, c->h_ldr_pinned.reserve((size_t)c->width * c->height * sizeof(uint32_t)));
    return JPT_OK;
}

// drain and destroy the pipeline slots' streams and the frame groups' helper streams (a borrowed helper is a slot's stream: it
// goes with the slot); the next render that needs them makes new ones
void release_streams(jpt_ctx* c)
{
    for (int k = 0; k < kMaxGroups - 1; k++) {
        hipStream_t& st = c->group_streams.aux_stream[k];
        if (st) {
            (void)hipStreamSynchronize(st);
            if (!c->aux_borrowed[k]) (void)hipStreamDestroy(st);
        }
        st = nullptr;
        c->aux_borrowed[k] = false;
    }
    for (PipeSlot& ps : c->slot) {
        if (ps.stream) {
            (void)hipStreamSynchronize(ps.stream);
            (void)hipStreamDestroy(ps.stream);
        }
        ps.stream = nullptr;
        ps.acc_done_valid = false;
    }
}

}  // namespace

// Blocking read-backs (jpt_read_ldr_rgba8 / accum_f32 / depth_f32): device -> the context's pinned read buffer -> the caller's
// memory.  A device-to-host copy straight into pageable memory runs at ~3 GB/s (8 MB of display image: 2.7 ms; 33 MB of float4
// sums: 11 ms); through pinned memory the copy runs at the link's rate and the host copy at memory speed.  (A buffer of its
// own: the split read-back's staging buffer may hold an image in flight.)
int jpt::staged_read(jpt_ctx* c, const void* src, size_t bytes)
{
    HIP_TRY(c, c->h_read_pinned.reserve(bytes));
    if (bytes) {
        HIP_TRY(c, hipMemcpyAsync(c->h_read_pinned.p, src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return JPT_OK;
}

int jpt::read_out(jpt_ctx* c, const void* src, size_t bytes, void* out)
{
    const int rc = staged_read(c, src, bytes);
    if (rc == JPT_OK && bytes) std::memcpy(out, c->h_read_pinned.p, bytes);
    return rc;
}

int jpt::read_rows_out(jpt_ctx* c, const void* src, size_t elem, int comps, bool whole, void* out)
{
    const size_t px_bytes = elem * (size_t)comps, full = (size_t)c->width * c->height * px_bytes;
    if (whole || c->world == 1) return read_out(c, src, whole ? full : (size_t)c->local_rows * c->width * px_bytes, out);
    const int rc = staged_read(c, src, (size_t)c->local_rows * c->width * px_bytes);
    if (rc != JPT_OK) return rc;
    std::memset(out, 0, full);
    scatter_rows(c->h_read_pinned.as<const char>(), static_cast<char*>(out), c->width, c->height, c->rank, c->world, (int)px_bytes);
    return JPT_OK;
}

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
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
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
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->trace_events) (void)hipEventDestroy(e);
    if (c->ev_readback) (void)hipEventDestroy(c->ev_readback);
    for (hipEvent_t e : c->primary.refl_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->enc_ev) if (e) (void)hipEventDestroy(e);
    if (c->ev_enc_readback) (void)hipEventDestroy(c->ev_enc_readback);
    c->upd.destroy_stream();
    release_streams(c);
    for (hipEvent_t e : c->group_streams.join) if (e) (void)hipEventDestroy(e);
    if (c->group_streams.fork) (void)hipEventDestroy(c->group_streams.fork);
    for (PipeSlot& ps : c->slot) {
        if (ps.ev_paths_done) (void)hipEventDestroy(ps.ev_paths_done);
        if (ps.ev_acc_done) (void)hipEventDestroy(ps.ev_acc_done);
    }
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
        for (PipeSlot& ps : c->slot) ps.acc_done_valid = false;
        c->stream = next;
    }
    return JPT_OK;
}

int jpt_renders_in_flight(const jpt_ctx* c) { return c ? c->last_pipe_slots : 0; }

int jpt_set_stream_priority(jpt_ctx* c, int32_t priority)
{
    if (!c) return JPT_E_INVALID;
    if (priority < JPT_STREAM_PRIORITY_DEFAULT || priority > JPT_STREAM_PRIORITY_LOW) return fail(c, JPT_E_INVALID, "unknown stream priority");
    if (priority == c->slot_priority) return JPT_OK;
    c->slot_priority = priority;
    if (c->device < 0) return JPT_OK;
    // the pipeline slots' streams are made on first use: drop the ones that exist, the next queued render makes new ones
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    release_streams(c);   // (the frame groups' helper streams follow them)
    c->six_queues = -1;   // (measured again for the new streams)
    return JPT_OK;
}

int jpt_set_memory_policy(jpt_ctx* c, int32_t renders_in_flight, uint64_t workspace_budget_bytes)
{
    if (!c) return JPT_E_INVALID;
    if (renders_in_flight < 0 || renders_in_flight > jpt_ctx::kPipeSlots) return fail(c, JPT_E_INVALID, "renders_in_flight must be 0 (the library's rule) or 1..8");
    c->max_slots = renders_in_flight;
    c->workspace_budget = workspace_budget_bytes;
    if (c->device < 0) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // drain, then give back what the new policy no longer allows: the workspaces of slots past the cap, and any workspace
    // larger than the new budget (the next render allocates what it needs)
    for (const PipeSlot& ps : c->slot)
        if (ps.stream) HIP_TRY(c, hipStreamSynchronize(ps.stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int keep = renders_in_flight > 0 ? renders_in_flight : jpt_ctx::kPipeSlots;
    for (int k = 0; k < jpt_ctx::kPipeSlots; k++) {
        PipeSlot& ps = c->slot[k];
        if (k >= keep || (workspace_budget_bytes && ps.workspace.n > workspace_budget_bytes)) {
            ps.workspace.release();
            ps.acc_done_valid = false;
        }
    }
    c->async_seq = 0;   // the next queued render starts at slot 0 again
    release_read_staging(c);   // (the pinned staging of the blocking read-backs: re-made by the next one)
    return JPT_OK;
}

int jpt_get_workspace_bytes(jpt_ctx* c, uint64_t* bytes_out)
{
    if (!c || !bytes_out) return JPT_E_INVALID;
    uint64_t n = 0;
    for (const PipeSlot& ps : c->slot) n += ps.workspace.n;
    *bytes_out = n;
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

int jpt_set_params(jpt_ctx* c, int32_t width, int32_t height, int32_t max_bounces, int32_t accum_mode, int32_t sampler_mode)
{
    if (!c) return JPT_E_INVALID;
    if (width < 0 || height < 0 || width > 65536 || height > 65536) return fail(c, JPT_E_INVALID, "bad resolution");
    if (max_bounces < 0 || max_bounces > kMaxBounces) return fail(c, JPT_E_INVALID, "max_bounces must be in [0,64]");
    if (accum_mode != JPT_ACCUM_REF_LDR8 && accum_mode != JPT_ACCUM_HDR_F32) return fail(c, JPT_E_INVALID, "unknown accum_mode");
    if (sampler_mode < JPT_SAMPLER_NEAREST_CLAMP || sampler_mode > JPT_SAMPLER_LINEAR_REPEAT) return fail(c, JPT_E_INVALID, "unknown sampler_mode");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no framebuffers");
    HIP_TRY(c, hipSetDevice(c->device));
    if (width != c->width || height != c->height) {
        // the post stages' images are of the old size: given back once the work that uses them has run
        if (c->post.sized_buffers()) HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->post.framebuffers_remade(true);
        c->primary.sh_valid = c->primary.refl_valid = false;   // (jpt_probe_project's coefficients and jpt_reflection_prefilter's chain likewise)
        // the temporal history is of the old size too (a new TemporalReprojection object): zeros at the next pass, and nothing to
        // read until then -- the pixel count alone does not tell (32 x 32 -> 16 x 64), and hist_written is sized by the old one
        c->hist_valid = false;
        c->hist_written = nullptr;
    }
    c->width = width;
    c->height = height;
    c->max_bounces = max_bounces;
    c->accum_mode = accum_mode;
    c->sampler_mode = sampler_mode;
    c->ds.sampler_mode = sampler_mode;
    c->params_set = true;
    c->depth_valid = false;
    return alloc_framebuffers(c);
}

int jpt_set_partition(jpt_ctx* c, int32_t rank, int32_t world)
{
    if (!c) return JPT_E_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, JPT_E_INVALID, "need 0 <= rank < world");
    c->rank = rank;
    c->world = world;
    if (c->params_set && c->device >= 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        return alloc_framebuffers(c);
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

int jpt_render(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index) { return do_render(c, n_frames, first_frame_index, false, true); }
int jpt_render_counted(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index) { return do_render(c, n_frames, first_frame_index, true, true); }
int jpt_render_async(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index) { return do_render(c, n_frames, first_frame_index, false, false); }

int jpt_sync(jpt_ctx* c)
{
    if (!c || c->device < 0) return JPT_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->stats.last_render_ms = c->stats.last_trace_ms = ms;
    else (void)hipGetLastError();   // (no render recorded yet -- queries alone: not an error to leave behind for the host's next HIP call)
    if (c->kernel_variant != JPT_KERNEL_REFERENCE_LAYOUT && c->trace_events_used > 0) c->stats.last_trace_ms = traced_ms(c, nullptr);
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

int jpt_set_kernel_timing(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    c->kernel_timing = enable != 0;
    if (!c->kernel_timing) c->trace_events_used = 0;
    return JPT_OK;
}

int jpt_accum_reset(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    c->frame_count = 0;  // frame_count == 1 on the next frame overwrites the sum (progressive_rendering.glsl:34)
    c->accum_restarts++;
    c->stats.frames = 0;
    c->assembled = c->assembled_ldr = false;
    c->hist_valid = false;  // temporal mode: history images start from zero again (a new TemporalReprojection object)
    c->hist_written = nullptr;   // (and jpt_read_accum_f32 has nothing to show until a pass has run)
    return JPT_OK;
}

int jpt_set_progressive_frame_count(jpt_ctx* c, uint32_t next_frame_count)
{
    if (!c) return JPT_E_INVALID;
    if (next_frame_count == 0) return fail(c, JPT_E_INVALID, "frame_count starts at 1 (progressive_rendering.cpp:20)");
    c->frame_count = next_frame_count - 1u;
    c->accum_restarts++;
    c->stats.frames = c->frame_count;
    c->assembled = c->assembled_ldr = false;
    return JPT_OK;
}

int jpt_set_denoising_mode(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_DENOISE_PROGRESSIVE && mode != JPT_DENOISE_TEMPORAL && mode != JPT_DENOISE_NONE)
        return fail(c, JPT_E_INVALID, "unknown denoising mode");
    if (mode != c->denoise) {
        // the modes do not share state: the progressive sum and the temporal history both start over
        c->frame_count = 0;
        c->accum_restarts++;
        c->stats.frames = 0;
        c->hist_valid = false;
        c->hist_written = nullptr;
        c->assembled = c->assembled_ldr = false;
    }
    c->denoise = mode;
    return JPT_OK;
}

int jpt_set_outputs(jpt_ctx* c, uint32_t outputs)
{
    if (!c) return JPT_E_INVALID;
    if (outputs & ~(uint32_t)JPT_OUTPUT_DEPTH) return fail(c, JPT_E_INVALID, "jpt_set_outputs: unknown output bit");
    c->outputs = outputs;   // (takes effect with the next render; a depth image already written stays readable until then)
    return JPT_OK;
}

int jpt_set_temporal_params(jpt_ctx* c, const void* render_parameters)
{
    if (!c) return JPT_E_INVALID;
    if (!render_parameters) return fail(c, JPT_E_INVALID, "null RenderParameters");
    std::memcpy(&c->temporal, render_parameters, sizeof(RefTemporalParams));
    c->temporal_set = true;
    return JPT_OK;
}

static int read_common(jpt_ctx* c, void* out)
{
    if (!c || !out) return fail(c, JPT_E_INVALID, "null output");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return JPT_OK;
}

int jpt_read_ldr_rgba8(jpt_ctx* c, uint8_t* out)
{
    const int rc = read_common(c, out);
    if (rc) return rc;
    // What the reference does every frame (get_image_uniform_buffer, path_tracing_camera.cpp:228-229): through staged_read.
    const bool whole = c->assembled || c->assembled_ldr;
    return read_rows_out(c, whole ? c->d_full_ldr.p : c->d_ldr.p, sizeof(uint32_t), 1, whole, out);
}

int jpt_readback_ldr_begin(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    if (c->readback_pending) return fail(c, JPT_E_STATE, "a read-back is already in flight (call jpt_readback_ldr_end)");
    HIP_TRY(c, hipSetDevice(c->device));
    c->readback_full = c->assembled || c->assembled_ldr;
    const size_t px = c->readback_full ? (size_t)c->width * c->height : (size_t)c->local_rows * c->width;
    {
        const int rc = ensure_ldr_pinned(c);
        if (rc) return rc;
    }
    if (!c->ev_readback) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_readback, hipEventDisableTiming));
    if (px)
        HIP_TRY(c, hipMemcpyAsync(c->h_ldr_pinned.p, c->readback_full ? c->d_full_ldr.p : c->d_ldr.p, px * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_readback, c->stream));
    c->readback_pending = true;
    return JPT_OK;
}

int jpt_readback_ldr_end(jpt_ctx* c, uint8_t* out)
{
    if (!c || !out) return fail(c, JPT_E_INVALID, "null output");
    if (!c->readback_pending) return fail(c, JPT_E_STATE, "no read-back in flight (call jpt_readback_ldr_begin)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->ev_readback));
    c->readback_pending = false;
    const size_t full = (size_t)c->width * c->height;
    if (c->readback_full || c->world == 1) {
        std::memcpy(out, c->h_ldr_pinned.p, full * 4);
    } else {
        std::memset(out, 0, full * 4);
        scatter_rows(c->h_ldr_pinned.as<const uint32_t>(), reinterpret_cast<uint32_t*>(out), c->width, c->height, c->rank, c->world, 1);
    }
    return JPT_OK;
}

int jpt_read_accum_f32(jpt_ctx* c, float* out)
{
    const int rc = read_common(c, out);
    if (rc) return rc;
    if (c->denoise == JPT_DENOISE_TEMPORAL) {
        // the rgba32f image of this mode is the history image the last pass wrote
        if (!c->hist_written) return fail(c, JPT_E_STATE, "no temporal pass has run since the last reset");
        return read_out(c, c->hist_written, (size_t)c->width * c->height * sizeof(float4), out);
    }
    return read_rows_out(c, c->assembled ? c->d_full_accum.p : c->d_accum.p, sizeof(float), 4, c->assembled, out);
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
    char* h = c->h_read_pinned.as<char>();
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
    HIP_TRY(c, c->h_read_pinned.reserve(cap * (sizeof(jpt_ray_hit) + 1)));
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

int jpt_read_depth_f32(jpt_ctx* c, float* out)
{
    int rc = read_common(c, out);
    if (rc) return rc;
    if (!c->depth_valid)
        return fail(c, JPT_E_STATE, (c->outputs & JPT_OUTPUT_DEPTH) ? "no render has written the depth image yet"
                                                                     : "the depth image is switched off (jpt_set_outputs): no render writes it");
    return read_rows_out(c, c->d_depth.p, sizeof(float), 1, false, out);
}

void* jpt_device_accum(jpt_ctx* c, size_t* bytes_out)
{
    if (!c) return nullptr;
    if (bytes_out) *bytes_out = c->d_accum.n * sizeof(float4);
    return c->d_accum.p;
}

void* jpt_device_ldr(jpt_ctx* c, size_t* bytes_out)
{
    if (!c) return nullptr;
    if (bytes_out) *bytes_out = c->d_ldr.n * sizeof(uint32_t);
    return c->d_ldr.p;
}

int32_t jpt_local_rows(jpt_ctx* c) { return c ? c->local_rows : 0; }

int jpt_assemble_from_ranks(jpt_ctx* c, const void* device_gathered, int32_t world)
{
    if (!c || !device_gathered) return fail(c, JPT_E_INVALID, "null gathered buffer");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    if (world != c->world) return fail(c, JPT_E_INVALID, "world differs from jpt_set_partition");
    if (c->denoise != JPT_DENOISE_PROGRESSIVE)
        return fail(c, JPT_E_STATE, "assembling re-derives the progressive display image; the other denoising modes run on one context");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t full = (size_t)c->width * c->height;
    HIP_TRY(c, c->d_full_accum.resize(full));
    HIP_TRY(c, c->d_full_ldr.resize(full));
    launch_assemble(c->stream, (const float4*)device_gathered, c->d_accum.p, c->rank, world, c->width, c->height,
                    max_rows_of_any_rank(c->height, world), c->d_full_accum.p, c->d_full_ldr.p, c->frame_count);
    HIP_TRY(c, hipGetLastError());
    c->assembled = true;  // asynchronous on the context's stream; jpt_read_* / jpt_sync wait for it
    return JPT_OK;
}

int jpt_assemble_ldr_from_ranks(jpt_ctx* c, const void* device_gathered, int32_t world)
{
    if (!c || !device_gathered) return fail(c, JPT_E_INVALID, "null gathered buffer");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    if (world != c->world) return fail(c, JPT_E_INVALID, "world differs from jpt_set_partition");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_full_ldr.resize((size_t)c->width * c->height));
    launch_assemble_ldr(c->stream, (const uint32_t*)device_gathered, c->d_ldr.p, c->rank, world, c->width, c->height,
                        max_rows_of_any_rank(c->height, world), c->d_full_ldr.p);
    HIP_TRY(c, hipGetLastError());
    c->assembled_ldr = true;  // asynchronous on the context's stream; jpt_read_ldr_rgba8 / jpt_sync wait for it
    return JPT_OK;
}

int jpt_get_stats(jpt_ctx* c, jpt_stats* out)
{
    if (!c || !out) return JPT_E_INVALID;
    *out = c->stats;
    return JPT_OK;
}

}  // extern "C"
