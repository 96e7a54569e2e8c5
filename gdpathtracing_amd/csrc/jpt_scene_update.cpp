// jpt_scene_update.cpp -- the calls that change a committed scene on the device without a new commit (jpt_scene_refit_tlas, jpt_scene_rebuild_tlas,
// jpt_scene_update_mesh, jpt_scene_rebuild_mesh, jpt_scene_set_mesh_rig, jpt_scene_clear_mesh_rig, jpt_scene_pose_mesh, jpt_scene_pose_mesh_rebuild) and the two that read their results (jpt_debug_mesh_records,
// jpt_debug_tlas_records), over SceneUpdates (jpt_ctx.h).  The host route (jpt_scene_update_tlas) is jpt_scene.cpp's, with the uploads it is made of
// and the refusals these calls open with (needs_scene, on_device).
#include "jpt_ctx.h"

#include <cfloat>
#include <chrono>
#include <cstring>

#include "jpt_instance_math.h"
#include "jpt_mesh_math.h"
#include "jpt_mesh_rebuild.h"

namespace {

// The refit stream and the events that order device refits against renders (jpt_scene_refit_tlas, jpt_scene_update_mesh)
int ensure_refit_stream(jpt_ctx* c)
{
    if (!c->upd.refit_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->upd.refit_stream, hipStreamNonBlocking));
    for (int k = 0; k < kInstanceSets; k++)
        if (!c->upd.ev_set_retired[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->upd.ev_set_retired[k], hipEventDisableTiming));
    if (!c->upd.ev_refit_done) HIP_TRY(c, hipEventCreateWithFlags(&c->upd.ev_refit_done, hipEventDisableTiming));
    return JPT_OK;
}

// The template of jpt_scene_rebuild_tlas for `n` instances (jpt_tlas_rebuild.h) with its refit schedule and stack need, on the host
// and on the device, and the sort's buffers: made at the first rebuild of this instance count (the host waits for the copies, once)
// and kept.  A count that changes comes with a new scene, whose upload the refit stream has long finished for; it is drained all the same.
int ensure_tlas_template(jpt_ctx* c, uint32_t n)
{
    if (c->upd.tlas_tmpl.n != n) {
        make_tlas_template(n, c->upd.tlas_tmpl);
        std::vector<uint32_t> identity(n);
        for (uint32_t i = 0; i < n; i++) identity[i] = i;
        std::vector<WideNode4> records;
        tlas_template_records(c->upd.tlas_tmpl, identity.data(), records);
        c->upd.tmpl_order_h.clear();
        c->upd.tmpl_levels_h.assign(1, 0u);
        refit4_schedule(records, 0, c->upd.tmpl_order_h, c->upd.tmpl_levels_h);
        c->upd.tmpl_stack_need = stack_need4_under(records, 0);
        HIP_TRY(c, hipStreamSynchronize(c->upd.refit_stream));
        c->upd.d_tmpl_child.release();   // (made again below)
    }
    if (c->upd.d_tmpl_child.p) return JPT_OK;
    hipStream_t rs = c->upd.refit_stream;
    HIP_TRY(c, c->upd.d_tmpl_child.upload(c->upd.tlas_tmpl.child, rs));
    HIP_TRY(c, c->upd.d_tmpl_order.upload(c->upd.tmpl_order_h, rs));
    HIP_TRY(c, c->upd.d_tmpl_levels.upload(c->upd.tmpl_levels_h, rs));
    HIP_TRY(c, c->upd.d_tlas_sorted.resize(n));
    HIP_TRY(c, c->upd.d_tlas_sort_keys.resize(n > kTlasLdsKeys ? 2 * (size_t)n : 0));
    HIP_TRY(c, hipStreamSynchronize(rs));   // pageable host vectors
    return JPT_OK;
}

// The other copies of the instance level, made at the first refit (or mesh rebuild) since the last host upload
int ensure_instance_copies(jpt_ctx* c)
{
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    if (!c->upd.set_b_ready) {
        // the other copies of the instance arrays start as copies of copy 0
        // (the TLAS tails were all uploaded).  Once per upload, so the drain does not matter.
        HIP_TRY(c, hipStreamSynchronize(s));
        const SceneBufs::InstanceSet& first = b.set[0];
        for (int k = 1; k < kInstanceSets; k++) {
            SceneBufs::InstanceSet& to = b.set[k];
            HIP_TRY(c, to.inst.resize(first.inst.n));
            HIP_TRY(c, to.winst4.resize(first.winst4.n));
            HIP_TRY(c, hipMemcpyAsync(to.inst.p, first.inst.p, first.inst.n * sizeof(RefInstance), hipMemcpyDeviceToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(to.winst4.p, first.winst4.p, first.winst4.n * sizeof(WideInstance), hipMemcpyDeviceToDevice, s));
            HIP_TRY(c, to.reach.resize(first.reach.n));
            if (first.reach.n)
                HIP_TRY(c, hipMemcpyAsync(to.reach.p, first.reach.p, first.reach.n * sizeof(ReachInst), hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(c, hipStreamSynchronize(s));
        c->upd.set_b_ready = true;
        for (bool& v : c->upd.set_retired_valid) v = false;
    }
    return JPT_OK;
}

// Instance records and TLAS boxes from the transforms at `dev_view` (n_instances x 12 floats the device can read), written into the
// copy of the instance level that new renders do not read yet, on the refit stream; the context's stream and every render queued
// from now on wait for it (refit_wait_seq).  The BLAS root boxes are read from the reference-layout nodes.
// `rebuild_sorted` (jpt_scene_rebuild_tlas; ensure_tlas_template has run): the copy also gets a new topology, the template's over the
// instances sorted on the device, and the host's mirror of the records (c->scene.wide, the schedule) becomes the template over
// rebuild_sorted, boxes not yet refitted.  Every later refit then runs over the template's schedule, and one into a copy whose tail
// still holds an older topology first copies the current copy's tail.
int queue_instance_refit(jpt_ctx* c, const float* dev_view, uint32_t n_instances, const uint32_t* rebuild_sorted = nullptr)
{
    lights_stale(c, false);
    if (const int rc = ensure_instance_copies(c); rc != JPT_OK) return rc;
    hipStream_t s = c->stream;
    SceneBufs& b = c->dev;
    // The refit writes the copy that new renders do not read yet (`next`); its last readers are the renders queued
    // before the refit that retired it, i.e. before ev_set_retired[next] was recorded on the context's stream (which
    // waits for every render).  The renders queued since read the current copy and keep running meanwhile.
    const int next = (c->upd.cur_set + 1) % kInstanceSets;
    HIP_TRY(c, hipEventRecord(c->upd.ev_set_retired[c->upd.cur_set], s));
    c->upd.set_retired_valid[c->upd.cur_set] = true;
    hipStream_t rs = c->upd.refit_stream;
    if (c->upd.set_retired_valid[next]) HIP_TRY(c, hipStreamWaitEvent(rs, c->upd.ev_set_retired[next], 0));
    const bool cuts = c->scene.ref.inst_cut_range.size() == 2 * (size_t)n_instances && !c->scene.ref.inst_cut_boxes.empty();
    Tlas4RefitArgs a;
    a.transforms12 = dev_view;
    a.n_instances = n_instances;
    a.bvh = b.bvh.p;
    a.instances = b.set[next].inst.p;
    a.wide_instances4 = b.set[next].winst4.p;
    a.reach = c->ds.reach_tri ? b.set[next].reach.p : nullptr;
    a.cut_boxes = cuts ? b.cut_boxes.p : nullptr;
    a.cut_range = cuts ? b.cut_range.p : nullptr;
    a.nodes4 = b.nodes4.p;
    a.nodesq = b.nodesq.p;
    a.n_blas_records = (uint32_t)c->upd.tail_first(c->scene.wide, next);
    if (rebuild_sorted) {
        WideScene& w = c->scene.wide;
        const uint32_t blas_need = w.stack_need4 - 1u - stack_need4_under(w.tlas_nodes4, w.tlas_root4);
        tlas_template_records(c->upd.tlas_tmpl, rebuild_sorted, w.tlas_nodes4);
        w.tlas_root4 = 0;
        w.stack_need4 = c->upd.tmpl_stack_need + 1u + blas_need;
        c->upd.tlas4_order_h = c->upd.tmpl_order_h;
        c->upd.tlas4_levels_h = c->upd.tmpl_levels_h;
        c->upd.topo_rebuilt = true;
        c->upd.set_topo_gen[next] = ++c->upd.topo_gen;
        a.rebuild_child = c->upd.d_tmpl_child.p;
        a.sorted = c->upd.d_tlas_sorted.p;
        a.sort_scratch = c->upd.d_tlas_sort_keys.p;
    } else if (c->upd.set_topo_gen[next] != c->upd.topo_gen) {
        a.copy_tail = true;
        a.copy_from = (uint32_t)c->upd.tail_first(c->scene.wide, c->upd.cur_set);
        c->upd.set_topo_gen[next] = c->upd.topo_gen;
    }
    a.n_tlas_records = (uint32_t)c->scene.wide.tlas_nodes4.size();
    a.order = c->upd.topo_rebuilt ? c->upd.d_tmpl_order.p : c->upd.d_tlas4_order.p;
    a.level_start = c->upd.topo_rebuilt ? c->upd.d_tmpl_levels.p : c->upd.d_tlas4_levels.p;
    a.n_levels = (uint32_t)c->upd.tlas4_levels_h.size() - 1u;
    launch_tlas4_refit(rs, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->upd.ev_refit_done, rs));
    // the context's stream (blocking renders, read-backs, uploads, foreign work) is ordered after the refit; queued
    // renders wait for it on their own streams (do_render_batch), not through the context's stream
    HIP_TRY(c, hipStreamWaitEvent(s, c->upd.ev_refit_done, 0));
    c->upd.refit_wait_seq++;
    c->upd.cur_set = next;
    set_scene_view(c);
    return JPT_OK;
}

// The device moved ahead of the host's mirrors (c->scene.ref, c->scene.wide) and of the other kernels' arrays, until the next upload.  `boxes_mirrored`:
// the host's TLAS boxes were refitted along, so the sky cull (compute_sky_cull) may go on reading them.
void device_ahead(jpt_ctx* c, bool boxes_mirrored)
{
    c->upd.cull_boxes_current = boxes_mirrored;
    c->upd.refit_active = true;
    c->ds.x.tlas_current = false;   // the copy of the reference's instance level is the last HOST update's: until the next one exact ties are decided inside one instance only (jpt_tie_walk.h)
}

// jpt_scene_refit_tlas and jpt_scene_rebuild_tlas (`rebuild`; `call`: the name for the state message): the same checks, staging and
// side effects; the rebuild also gives the copy it writes a new topology
int move_instances(jpt_ctx* c, const float* transforms12, uint32_t n_instances, bool rebuild, const char* call)
{
    if (const int rc = needs_scene(c, kNativeTree, call, " needs a scene made by jpt_scene_commit with the native builder"); rc != JPT_OK) return rc;
    if (!transforms12 && n_instances) return fail(c, JPT_E_INVALID, "null transforms");
    if (n_instances != c->scene.ref.instances.size()) return fail(c, JPT_E_INVALID, "one transform per instance of the committed scene");
    if (const int rc = on_device(c, "host-only context: the refit runs on the device (jpt_scene_update_tlas is the host route)", false); rc != JPT_OK) return rc;
    // the host keeps the transforms (a later jpt_scene_update_tlas rebuilds from them); its arrays are stale from here on
    for (uint32_t i = 0; i < n_instances; i++) (void)c->scene.builder.set_instance_transform(i, transforms12 + (size_t)i * 12);
    c->scene.tlas_dirty = true;
    if (!c->ds.use4 || !c->scene.device_ready) return jpt_scene_update_tlas(c);  // no four-child records to refit
    if (n_instances == 0) return JPT_OK;
    if (n_instances <= 1) rebuild = false;   // one instance is its own order
    if (rebuild && n_instances > kTlasRebuildMaxInstances)
        return fail(c, JPT_E_LIMIT, "jpt_scene_rebuild_tlas sorts at most " + std::to_string(kTlasRebuildMaxInstances) + " instances");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_refit_stream(c);
    if (rc != JPT_OK) return rc;
    // The host's side of a rebuild, before anything is written.  For a modest number of instances the host repeats the sort on its
    // own root-rule boxes (the mirror below): its order may differ from the device's, whose boxes are tightened by the cuts, but
    // every instance is under the mirror's root, which is all the sky cull asks.  Beyond that the mirror's leaves are in index order
    // and the cull is off.
    const bool mirror = n_instances <= 4096u && !c->upd.mesh_deformed;
    std::vector<RefInstance> boxes;
    if (mirror) {
        boxes.resize(n_instances);
        for (uint32_t i = 0; i < n_instances; i++) {
            const RefBvhNode& root = c->scene.ref.bvh_nodes[c->scene.ref.instances[i].blas_index];
            instance_record(transforms12 + (size_t)i * 12, root.aabbMin, root.aabbMax, true, boxes[i]);
        }
    }
    std::vector<uint32_t> sorted;
    if (rebuild) {
        rc = ensure_tlas_template(c, n_instances);
        if (rc != JPT_OK) return rc;
        const WideScene& w = c->scene.wide;
        const uint32_t need = w.stack_need4 - stack_need4_under(w.tlas_nodes4, w.tlas_root4) + c->upd.tmpl_stack_need;
        if (need > trace_stack_capacity()) return too_deep(c, need, " after the TLAS rebuild");
        sorted.resize(n_instances);
        if (mirror) tlas_order_host(&boxes[0].aabbMin.x, &boxes[0].aabbMax.x, sizeof(RefInstance) / sizeof(float), n_instances, nullptr, sorted.data());
        else
            for (uint32_t i = 0; i < n_instances; i++) sorted[i] = i;
    }
    const size_t bytes = (size_t)n_instances * 12 * sizeof(float);
    int st = 0;
    HIP_TRY(c, c->upd.refit_stage.next(bytes, st));
    std::memcpy(c->upd.refit_stage.buf[st].p, transforms12, bytes);
    // the kernel reads the transforms straight from the pinned buffer (48 B per instance over the host link)
    float* dev_view = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer((void**)&dev_view, c->upd.refit_stage.buf[st].p, 0));
    rc = queue_instance_refit(c, dev_view, n_instances, rebuild ? sorted.data() : nullptr);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->upd.refit_stage.copied[st], c->upd.refit_stream));
    // The sky cull (compute_sky_cull) projects the boxes the TLAS root offers, on the host.  For a modest number of
    // instances the host repeats the TLAS refit on its own copy of the four-child TLAS records (refit_slots, same schedule:
    // ~0.1 us per instance), over instance boxes by the root rule alone: without the cut tightening the device applies, so its
    // boxes contain the device's (safe for the cull) but are looser.  Beyond that the cull is off until the next
    // jpt_scene_update_tlas.  After jpt_scene_update_mesh the host's root boxes are the committed vertices': off until the next
    // jpt_scene_commit.
    const bool mirrored = mirror && !c->upd.tlas4_levels_h.empty();
    if (mirrored) {
        WideScene& w = c->scene.wide;
        for (size_t l = 0; l + 1 < c->upd.tlas4_levels_h.size(); l++)
            for (uint32_t k = c->upd.tlas4_levels_h[l]; k < c->upd.tlas4_levels_h[l + 1]; k++)
                refit_slots(w.tlas_nodes4[c->upd.tlas4_order_h[k]], w.tlas_nodes4.data(), [&](int32_t ref, float* lo, float* hi) {
                    const RefInstance& in = boxes[(uint32_t)~ref];
                    lo[0] = in.aabbMin.x; lo[1] = in.aabbMin.y; lo[2] = in.aabbMin.z;
                    hi[0] = in.aabbMax.x; hi[1] = in.aabbMax.y; hi[2] = in.aabbMax.z;
                });
    }
    device_ahead(c, mirrored);
    c->stats.last_build_ms = ms_since(t0);
    return JPT_OK;
}

// Per mesh: where its records and triangles are on the device and the bottom-up schedule of its records (refit4_schedule), with
// the triangles' vertex indices; made and uploaded at the first jpt_scene_update_mesh after an upload (once per upload: the
// host waits for the copies).  Every call that needs them is about to work on the device: it is made current first.
int ensure_mesh_refit(jpt_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->upd.mesh_refit_ready) return JPT_OK;
    const RefScene& r = c->scene.ref;
    const WideScene& w = c->scene.wide;
    const size_t n_meshes = r.mesh_roots.size();
    if (r.mesh_tri_range.size() != 2 * n_meshes || r.tri_vidx.size() != 3 * r.tri_geom.size() || w.instances4.size() != r.instances.size())
        return fail(c, JPT_E_STATE, "the scene holds no vertex map for device updates: commit it again with JPT_BUILD_SAH_WATERTIGHT");
    c->upd.mesh_refit.assign(n_meshes, SceneUpdates::MeshRefit{});
    c->upd.mesh_order_h.clear();
    c->upd.mesh_levels_h.clear();
    for (size_t m = 0; m < n_meshes; m++) {
        SceneUpdates::MeshRefit& mr = c->upd.mesh_refit[m];
        mr.bvh_root = r.mesh_roots[m];
        mr.tri_first = r.mesh_tri_range[2 * m];
        mr.n_tris = r.mesh_tri_range[2 * m + 1];
        if (mr.n_tris == 0) continue;   // (an empty mesh stands for another mesh's tree: nothing of its own on the device)
        size_t inst = r.instances.size();
        for (size_t i = 0; i < r.instances.size(); i++)
            if (r.instances[i].blas_index == mr.bvh_root) {
                inst = i;
                break;
            }
        if (inst == r.instances.size()) continue;   // no instance names it: flatten made no tree for it
        mr.has_tree = true;
        mr.root4 = w.instances4[inst].root;
        mr.level_first = (uint32_t)c->upd.mesh_levels_h.size();
        const size_t order_first = c->upd.mesh_order_h.size();
        c->upd.mesh_levels_h.push_back((uint32_t)order_first);
        refit4_schedule(w.blas_nodes4, mr.root4, c->upd.mesh_order_h, c->upd.mesh_levels_h);
        mr.n_levels = (uint32_t)(c->upd.mesh_levels_h.size() - mr.level_first - 1);
        if (mr.root4 >= 0) {
            uint32_t lo = (uint32_t)mr.root4, hi = (uint32_t)mr.root4;
            for (size_t k = order_first; k < c->upd.mesh_order_h.size(); k++) {
                lo = std::min(lo, c->upd.mesh_order_h[k]);
                hi = std::max(hi, c->upd.mesh_order_h[k]);
            }
            mr.rec_first = lo;
            mr.n_recs = hi - lo + 1;
        }
    }
    const int rc = ensure_refit_stream(c);
    if (rc != JPT_OK) return rc;
    hipStream_t rs = c->upd.refit_stream;
    HIP_TRY(c, c->upd.d_tri_vidx.upload(r.tri_vidx, rs));
    HIP_TRY(c, c->upd.d_mesh_order.upload(c->upd.mesh_order_h, rs));
    HIP_TRY(c, c->upd.d_mesh_levels.upload(c->upd.mesh_levels_h, rs));
    HIP_TRY(c, hipStreamSynchronize(rs));   // pageable host vectors
    c->upd.mesh_refit_ready = true;
    return JPT_OK;
}

// The region of jpt_scene_rebuild_mesh for mesh `mesh_id` (ensure_mesh_refit has run; the mesh has a tree of two triangles or more).  At
// the mesh's first rebuild since the last upload: the template of its triangle count (make_tlas_template) with its schedule and
// stack need; JPT_E_LIMIT, before anything is written or reserved, when a traversal could then need more entries than the kernels
// hold; then -- the host waits for the queued renders and refits, once per mesh -- the record arrays grown by the template's records
// BEHIND the TLAS tails (every existing offset stays), the root word of the mesh's instances pointed at the region's record 0 in every
// copy of the instance level and in c->scene.wide.instances4, the template's child words, schedule and level starts uploaded, the sort's
// working set sized, and mesh_refit[mesh_id] naming the region.  Later calls find all of it in place.
int ensure_mesh_region(jpt_ctx* c, uint32_t mesh_id, const char* call)
{
    SceneUpdates& u = c->upd;
    SceneUpdates::MeshRefit& mr = u.mesh_refit[mesh_id];
    if (mr.rebuilt) return u.mesh_regions.count(mesh_id) ? JPT_OK : fail(c, JPT_E_STATE, std::string(call) + ": the mesh's region left with its scene");
    WideScene& w = c->scene.wide;
    if (u.mesh_need.empty()) {
        std::vector<int32_t> roots(u.mesh_refit.size(), -1);   // (a leaf root, and a mesh without a tree: need 0)
        for (size_t m = 0; m < roots.size(); m++)
            if (u.mesh_refit[m].has_tree) roots[m] = u.mesh_refit[m].root4;
        stack_need4_each(w.blas_nodes4, roots, u.mesh_need);
    }
    TlasTemplate t;
    make_tlas_template(mr.n_tris, t);
    std::vector<uint32_t> order, levels(1, 0u);
    uint32_t need_own = 0;
    {
        std::vector<uint32_t> identity(mr.n_tris);
        for (uint32_t i = 0; i < mr.n_tris; i++) identity[i] = i;
        std::vector<WideNode4> records;
        tlas_template_records(t, identity.data(), records);
        refit4_schedule(records, 0, order, levels);
        need_own = stack_need4_under(records, 0);
    }
    uint32_t blas_old = 0, blas_new = need_own;
    for (size_t m = 0; m < u.mesh_need.size(); m++) {
        blas_old = std::max(blas_old, u.mesh_need[m]);
        if (m != mesh_id) blas_new = std::max(blas_new, u.mesh_need[m]);
    }
    const uint32_t need = w.stack_need4 - blas_old + blas_new;   // (stack_need4: the TLAS need + 1 + the largest mesh need)
    if (need > trace_stack_capacity()) return too_deep(c, need, " after the mesh rebuild");
    SceneBufs& b = c->dev;
    const size_t first = b.nodes4.n, total = first + t.n_records;
    if (b.nodesq.n != first || total > (size_t)0x7fffffff) return fail(c, JPT_E_LIMIT, std::string(call) + ": more records than a child word can name");
    int rc = ensure_refit_stream(c);
    if (rc != JPT_OK) return rc;
    hipStream_t s = c->stream, rs = u.refit_stream;
    // every render, read-back and refit queued so far holds the arrays' addresses (the context's stream follows them all)
    HIP_TRY(c, hipStreamSynchronize(rs));
    HIP_TRY(c, hipStreamSynchronize(s));
    {
        DevBuf<WideNode4> n4;
        DevBuf<WideNodeQ> nq;
        HIP_TRY(c, n4.resize(total));
        HIP_TRY(c, nq.resize(total));
        HIP_TRY(c, hipMemcpyAsync(n4.p, b.nodes4.p, first * sizeof(WideNode4), hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(nq.p, b.nodesq.p, first * sizeof(WideNodeQ), hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        std::swap(n4.p, b.nodes4.p);
        std::swap(n4.n, b.nodes4.n);
        std::swap(nq.p, b.nodesq.p);
        std::swap(nq.n, b.nodesq.n);
    }
    rc = ensure_instance_copies(c);
    if (rc != JPT_OK) return rc;
    const uint32_t n_inst = (uint32_t)c->scene.ref.instances.size();
    for (int k = 0; k < kInstanceSets; k++) launch_mesh_root_words(s, b.set[k].winst4.p, b.set[0].inst.p, n_inst, mr.bvh_root, (int32_t)first);
    HIP_TRY(c, hipGetLastError());
    for (uint32_t i = 0; i < n_inst; i++)
        if (c->scene.ref.instances[i].blas_index == mr.bvh_root) w.instances4[i].root = (int32_t)first;
    for (uint32_t& r : order) r += (uint32_t)first;
    SceneUpdates::MeshRegion& rg = u.mesh_regions[mesh_id];
    HIP_TRY(c, rg.d_child.upload(t.child, s));
    HIP_TRY(c, rg.d_order.upload(order, s));
    HIP_TRY(c, rg.d_levels.upload(levels, s));
    if (u.d_mesh_sort.n < mesh_sort_words(mr.n_tris)) HIP_TRY(c, u.d_mesh_sort.resize(mesh_sort_words(mr.n_tris)));
    HIP_TRY(c, hipStreamSynchronize(s));   // pageable host vectors
    rg.levels_h = levels;
    mr.root4 = (int32_t)first;
    mr.rec_first = (uint32_t)first;
    mr.n_recs = t.n_records;
    mr.level_first = 0;
    mr.n_levels = (uint32_t)levels.size() - 1u;
    mr.rebuilt = true;
    u.mesh_need[mesh_id] = need_own;
    w.stack_need4 = need;
    set_scene_view(c);
    return JPT_OK;
}

// The state and argument checks of a call that gives new arrays for a committed mesh (`call`: jpt_scene_update_mesh,
// jpt_scene_set_mesh_rig): a JPT_BUILD_SAH_WATERTIGHT commit, the mesh's own topology, normals for every surface or for none
// (with_normals: whether they came).  sv: the surfaces as the builder views them.
int check_mesh_arrays(jpt_ctx* c, const char* call, uint32_t mesh_id, const jpt_surface* surfaces, int32_t n_surfaces, std::vector<SurfaceView>& sv,
                      int& with_normals)
{
    const int rc = needs_scene(c, kWatertightTree, call, " needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT",
                               "the scene was committed with JPT_BUILD_REFERENCE_EXACT: its trees are the reference's own, which a refit "
                               "would not keep (commit with JPT_BUILD_SAH_WATERTIGHT to deform meshes on the device)",
                               "the scene was committed with JPT_BUILD_SAH: its reach records and tie shadow are the reference builder's "
                               "tree of the committed vertices (commit with JPT_BUILD_SAH_WATERTIGHT to deform meshes on the device)");
    if (rc != JPT_OK) return rc;
    if (mesh_id >= c->scene.builder.mesh_count()) return fail(c, JPT_E_INVALID, "no such mesh");
    if (n_surfaces < 0 || (n_surfaces && !surfaces)) return fail(c, JPT_E_INVALID, "bad surface array");
    sv.assign((size_t)n_surfaces, SurfaceView{});
    int with_vertices = 0;
    with_normals = 0;
    for (int32_t i = 0; i < n_surfaces; i++) {
        const jpt_surface& x = surfaces[i];
        if (x.n_vertices > 0) {
            if (!x.vertices) return fail(c, JPT_E_INVALID, "surface needs a vertex array");
            with_vertices++;
            with_normals += x.normals ? 1 : 0;
        }
        sv[(size_t)i] = SurfaceView{x.vertices, x.normals, nullptr, x.indices, x.n_vertices, x.n_indices};
    }
    if (!c->scene.builder.same_topology(mesh_id, sv.data(), n_surfaces)) return fail(c, JPT_E_INVALID, "topology changed: commit the scene again");
    if (with_normals != 0 && with_normals != with_vertices) return fail(c, JPT_E_INVALID, "give normals for every surface of the mesh or for none");
    return JPT_OK;
}

// One stage of mesh_stage as jpt_scene_update_mesh and jpt_scene_pose_mesh fill it: the same pinned bytes as the host (h) and the device see them
struct MeshStage {
    int index = 0;
    char *h = nullptr, *dev = nullptr;
};

// The next stage of mesh_stage for an update whose own parts end at `t_off`, with what every layout shares written: the 32-byte head
// (6 ordered keys + pad: the bounds the refit gathers) and, from t_off, the transforms of every instance, which the instance refit
// reads from the pinned buffer.  d_mesh_in grows to dev_bytes behind the refit stream's drain; ev_mesh_drain is made once.
int stage_mesh_update(jpt_ctx* c, size_t t_off, size_t dev_bytes, MeshStage& st)
{
    SceneUpdates& u = c->upd;
    const uint32_t n_inst = (uint32_t)c->scene.ref.instances.size();
    HIP_TRY(c, u.mesh_stage.next(t_off + (size_t)n_inst * 12 * sizeof(float), st.index));
    if (!u.ev_mesh_drain) HIP_TRY(c, hipEventCreateWithFlags(&u.ev_mesh_drain, hipEventDisableTiming));
    st.h = u.mesh_stage.buf[st.index].as<char>();
    const int32_t keys[8] = {ordered_key(FLT_MAX), ordered_key(FLT_MAX), ordered_key(FLT_MAX),
                             ordered_key(-FLT_MAX), ordered_key(-FLT_MAX), ordered_key(-FLT_MAX), 0, 0};
    std::memcpy(st.h, keys, sizeof keys);
    for (uint32_t i = 0; i < n_inst; i++) std::memcpy(st.h + t_off + (size_t)i * 48, c->scene.builder.instance_transform(i), 48);
    if (u.d_mesh_in.n < dev_bytes) {
        HIP_TRY(c, hipStreamSynchronize(u.refit_stream));   // (an earlier update may still read the old buffer)
        HIP_TRY(c, u.d_mesh_in.resize(dev_bytes));
    }
    HIP_TRY(c, hipHostGetDevicePointer((void**)&st.dev, st.h, 0));
    return JPT_OK;
}

// One pipeline drain on the device: the refit stream waits for every render queued so far (the context's stream follows them all)
hipError_t drain_pipeline(jpt_ctx* c)
{
    const hipError_t e = hipEventRecord(c->upd.ev_mesh_drain, c->stream);
    return e == hipSuccess ? hipStreamWaitEvent(c->upd.refit_stream, c->upd.ev_mesh_drain, 0) : e;
}

// What jpt_scene_update_mesh and jpt_scene_pose_mesh do once the mesh's new vertices (and normals, or null: they stay) are on their way
// into d_mesh_in behind its bounds head, on the refit stream and behind the pipeline drain: the mesh's records refitted from them,
// then the instance level over the new root boxes with the current transforms (`dev_transforms`: the stage's copy, as the device sees
// it), as jpt_scene_refit_tlas does; the stage `st` of mesh_stage is free again once all of it has run.
// `rebuild` (ensure_mesh_region has run for `mesh_id`): between the triangle records and the refit the region's records get a new
// topology, the template's over the mesh's triangles sorted on the device (jpt_kernels_mesh_rebuild.hip).
int queue_mesh_refit(jpt_ctx* c, uint32_t mesh_id, bool rebuild, const float* verts, const float* normals, const float* dev_transforms,
                     const MeshStage& st, std::chrono::steady_clock::time_point t0)
{
    const SceneUpdates::MeshRefit& mr = c->upd.mesh_refit[mesh_id];
    const SceneUpdates::MeshRegion* rg = nullptr;
    if (mr.rebuilt) {
        const auto it = c->upd.mesh_regions.find(mesh_id);
        if (it == c->upd.mesh_regions.end()) return fail(c, JPT_E_STATE, "the mesh's region left with its scene");
        rg = &it->second;
    }
    const uint32_t n_inst = (uint32_t)c->scene.ref.instances.size();
    MeshRefitArgs a;
    a.bounds = reinterpret_cast<int32_t*>(c->upd.d_mesh_in.p);
    a.verts = verts;
    a.normals = normals;
    a.vidx = c->upd.d_tri_vidx.p;
    a.tri_first = mr.tri_first;
    a.n_tris = mr.n_tris;
    const SceneBufs& b = c->dev;
    a.wtris = b.wtris.p;
    a.shade = b.shade_tris.p;
    a.nodes4 = b.nodes4.p;
    a.nodesq = b.nodesq.p;
    a.order = rg ? rg->d_order.p : c->upd.d_mesh_order.p;
    a.level_start = rg ? rg->d_levels.p : c->upd.d_mesh_levels.p + mr.level_first;
    a.root4 = mr.root4;
    a.bvh = b.bvh.p;
    a.bvh_root = mr.bvh_root;
    const bool cuts = c->scene.ref.inst_cut_range.size() == 2 * (size_t)n_inst && !c->scene.ref.inst_cut_boxes.empty();
    a.cut_range = cuts ? b.cut_range.p : nullptr;
    a.instances = b.set[0].inst.p;   // (blas_index is the same in every copy of the instance level)
    a.n_instances = n_inst;
    const uint32_t* h_levels = rg ? rg->levels_h.data() : c->upd.mesh_levels_h.data() + mr.level_first;
    if (rebuild && rg) {
        hipStream_t rs = c->upd.refit_stream;
        launch_mesh_tris(rs, a);
        MeshOrderArgs o;
        o.verts = verts;
        o.vidx = a.vidx;
        o.tri_first = mr.tri_first;
        o.n_tris = mr.n_tris;
        o.work = c->upd.d_mesh_sort.p;
        launch_mesh_order(rs, o);
        launch_tlas_template(rs, rg->d_child.p, mr.n_recs, mesh_order_sorted(o), a.nodes4, mr.rec_first);
        launch_mesh_records(rs, a, h_levels, mr.n_levels);
    } else {
        launch_mesh_refit(c->upd.refit_stream, a, h_levels, mr.n_levels);
    }
    HIP_TRY(c, hipGetLastError());
    // the instance level over the new root boxes, with the current transforms, as jpt_scene_refit_tlas does
    const int rc = queue_instance_refit(c, dev_transforms, n_inst);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->upd.mesh_stage.copied[st.index], c->upd.refit_stream));
    device_ahead(c, false);   // the host's TLAS boxes are stale: no sky cull until the next upload
    c->stats.last_build_ms = ms_since(t0);
    return JPT_OK;
}

}  // namespace

// The rigs of jpt_scene_set_mesh_rig leave with the scene they were set for (a queued pose may still read them: the refit stream first)
void jpt::drop_mesh_rigs(jpt_ctx* c)
{
    if (c->upd.mesh_rigs.empty() && c->upd.mesh_regions.empty()) return;
    if (c->device >= 0 && c->upd.refit_stream) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->upd.refit_stream);
    }
    c->upd.mesh_rigs.clear();
    c->upd.mesh_regions.clear();   // (the regions' records go with the record arrays, at the upload that follows: host_uploaded)
}

int jpt_scene_refit_tlas(jpt_ctx* c, const float* t12, uint32_t n) { return move_instances(c, t12, n, false, "jpt_scene_refit_tlas"); }
int jpt_scene_rebuild_tlas(jpt_ctx* c, const float* t12, uint32_t n) { return move_instances(c, t12, n, true, "jpt_scene_rebuild_tlas"); }

namespace {

// jpt_scene_update_mesh and jpt_scene_rebuild_mesh (`rebuild`; `call`: the name for the messages): the same checks, staging and side effects;
// the rebuild also gives the mesh's records a new topology (a mesh of fewer than two triangles is its own order: the refit)
int deform_mesh(jpt_ctx* c, uint32_t mesh_id, const jpt_surface* surfaces, int32_t n_surfaces, bool rebuild, const char* call)
{
    std::vector<SurfaceView> sv;
    int with_normals = 0;
    int rc = check_mesh_arrays(c, call, mesh_id, surfaces, n_surfaces, sv, with_normals);
    if (rc == JPT_OK) rc = on_device(c, "host-only context: the update runs on the device", true);
    if (rc != JPT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    rc = ensure_mesh_refit(c);
    if (rc != JPT_OK) return rc;
    const SceneUpdates::MeshRefit& mr = c->upd.mesh_refit[mesh_id];
    rebuild = rebuild && mr.has_tree && mr.n_tris >= 2;
    if (rebuild) rc = ensure_mesh_region(c, mesh_id, call);
    if (rc != JPT_OK) return rc;
    c->upd.mesh_deformed = true;   // (the host's arrays describe the committed vertices from here on)
    if (!mr.has_tree) return JPT_OK;   // no instance names the mesh: the device holds nothing of it
    // staging: [6 ordered keys + pad: 32 B][vertices][normals][transforms]; the first three parts are copied to the device, the
    // instance refit reads the transforms from the pinned buffer
    const size_t head = 32, vbytes = c->scene.builder.mesh_vertex_count(mesh_id) * 3 * sizeof(float), nbytes = with_normals ? vbytes : 0, dev_bytes = head + vbytes + nbytes;
    MeshStage st;
    rc = stage_mesh_update(c, dev_bytes, dev_bytes, st);
    if (rc != JPT_OK) return rc;
    size_t off = head;
    for (const SurfaceView& x : sv) {
        const size_t b = (size_t)x.n_vertices * 3 * sizeof(float);
        if (b) std::memcpy(st.h + off, x.vertices, b);
        if (b && with_normals) std::memcpy(st.h + off + vbytes, x.normals, b);
        off += b;
    }
    // The BLAS records, triangle records and root boxes are shared by every copy of the instance level: the update waits on the
    // device for every render queued before it (the context's stream follows them all) -- one pipeline drain.
    HIP_TRY(c, drain_pipeline(c));
    const char* in = c->upd.d_mesh_in.p;
    HIP_TRY(c, hipMemcpyAsync(c->upd.d_mesh_in.p, st.h, dev_bytes, hipMemcpyHostToDevice, c->upd.refit_stream));
    return queue_mesh_refit(c, mesh_id, rebuild, reinterpret_cast<const float*>(in + head), with_normals ? reinterpret_cast<const float*>(in + head + vbytes) : nullptr,
                            reinterpret_cast<const float*>(st.dev + dev_bytes), st, t0);
}

}  // namespace

int jpt_scene_update_mesh(jpt_ctx* c, uint32_t mesh_id, const jpt_surface* surfaces, int32_t n_surfaces)
{
    return deform_mesh(c, mesh_id, surfaces, n_surfaces, false, "jpt_scene_update_mesh");
}
int jpt_scene_rebuild_mesh(jpt_ctx* c, uint32_t mesh_id, const jpt_surface* surfaces, int32_t n_surfaces)
{
    return deform_mesh(c, mesh_id, surfaces, n_surfaces, true, "jpt_scene_rebuild_mesh");
}

int jpt_scene_set_mesh_rig(jpt_ctx* c, uint32_t mesh_id, const jpt_surface* bind, const jpt_surface_rig* rigs, int32_t n_surfaces, int32_t influences,
                           int32_t n_blend_shapes)
{
    std::vector<SurfaceView> sv;
    int with_normals = 0;
    int rc = check_mesh_arrays(c, "jpt_scene_set_mesh_rig", mesh_id, bind, n_surfaces, sv, with_normals);
    if (rc != JPT_OK) return rc;
    if (n_surfaces && !rigs) return fail(c, JPT_E_INVALID, "jpt_scene_set_mesh_rig: bad rig array");
    std::vector<SkinPiece> pieces((size_t)n_surfaces);
    for (int32_t i = 0; i < n_surfaces; i++) {
        SkinPiece& x = pieces[(size_t)i];
        x.n_vertices = bind[i].n_vertices;
        x.positions = bind[i].vertices;
        x.normals = bind[i].normals;
        x.bones = rigs[i].bones;
        x.weights = rigs[i].weights;
        x.dpos = rigs[i].position_deltas;
        x.dnrm = rigs[i].normal_deltas;
    }
    SkinRigInfo info;
    std::string why;
    rc = check_skin_rig("jpt_scene_set_mesh_rig", pieces.data(), n_surfaces, influences, n_blend_shapes, with_normals != 0, info, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    rc = on_device(c, "host-only context: the rig is kept on the device", true);
    if (rc == JPT_OK) rc = ensure_mesh_refit(c);
    if (rc == JPT_OK) rc = jpt_scene_clear_mesh_rig(c, mesh_id);   // (a queued pose may still read the rig this one replaces)
    if (rc != JPT_OK) return rc;
    SceneUpdates::MeshRig& rig = c->upd.mesh_rigs[mesh_id];
    rig.info = info;
    if (!c->upd.mesh_refit[mesh_id].has_tree || info.bytes == 0) return JPT_OK;   // no instance names the mesh: nothing of it on the device
    std::vector<char> block(info.bytes);
    pack_skin_rig(info, pieces.data(), n_surfaces, block.data());
    hipError_t e = rig.d_rig.resize(info.bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(rig.d_rig.p, block.data(), info.bytes, hipMemcpyHostToDevice, c->upd.refit_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->upd.refit_stream);   // pageable host memory
    if (e != hipSuccess) {
        c->upd.mesh_rigs.erase(mesh_id);
        return hip_fail(c, e, "jpt_scene_set_mesh_rig: the rig's copy");
    }
    return JPT_OK;
}

int jpt_scene_clear_mesh_rig(jpt_ctx* c, uint32_t mesh_id)
{
    if (!c) return JPT_E_INVALID;
    auto it = c->upd.mesh_rigs.find(mesh_id);
    if (it == c->upd.mesh_rigs.end()) return JPT_OK;
    if (it->second.d_rig.p) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (c->upd.refit_stream) HIP_TRY(c, hipStreamSynchronize(c->upd.refit_stream));   // (a queued pose may still read it)
    }
    c->upd.mesh_rigs.erase(it);
    return JPT_OK;
}

namespace {

// jpt_scene_pose_mesh and jpt_scene_pose_mesh_rebuild (`rebuild`; `call`: the name for the messages), as deform_mesh
int pose_mesh(jpt_ctx* c, uint32_t mesh_id, const float* bone_transforms12, uint32_t n_bones, const float* blend_weights, uint32_t n_blend_weights,
              bool rebuild, const char* call)
{
    // jpt_scene_update_mesh's state rules, on their own account: a rig is dropped with its scene, but a pose does not rely on that
    if (const int rc = needs_scene(c, kWatertightTree, call, " needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT"); rc != JPT_OK) return rc;
    auto it = c->upd.mesh_rigs.find(mesh_id);
    if (it == c->upd.mesh_rigs.end()) return fail(c, JPT_E_STATE, std::string(call) + ": the mesh has no rig (jpt_scene_set_mesh_rig; a commit or an upload drops it)");
    const SceneUpdates::MeshRig& rig = it->second;
    const SkinRigInfo& info = rig.info;
    std::vector<SkinShape> active;
    std::string why;
    int rc = check_skin_pose(call, info, bone_transforms12, n_bones, blend_weights, n_blend_weights, active, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    rc = on_device(c, "host-only context: the pose runs on the device", true);
    if (rc != JPT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    rc = ensure_mesh_refit(c);
    if (rc != JPT_OK) return rc;
    const SceneUpdates::MeshRefit& mr = c->upd.mesh_refit[mesh_id];
    // no instance names the mesh: the device holds nothing of it, nothing changes anywhere and the host's copy of the scene stays current
    if (!mr.has_tree || !rig.d_rig.p) return JPT_OK;
    rebuild = rebuild && mr.n_tris >= 2;
    if (rebuild) rc = ensure_mesh_region(c, mesh_id, call);
    if (rc != JPT_OK) return rc;
    c->upd.mesh_deformed = true;   // (as jpt_scene_update_mesh: the host's arrays describe the committed vertices from here on)
    // staging: [6 ordered keys + pad: 32 B][palette: the bones the rig can name][active shapes, padded to 16 B][transforms]; the first
    // three parts are copied to the head of d_mesh_in, where the vertices and normals the skin kernel writes follow them
    const uint32_t n_pal = info.influences ? (uint32_t)(info.max_bone + 1) : 0u;
    const size_t head = 32, pbytes = (size_t)n_pal * 48, abytes = (active.size() * sizeof(SkinShape) + 15u) & ~(size_t)15u;
    const size_t in_bytes = head + pbytes + abytes, vbytes = ((size_t)info.n_vertices * 3 * sizeof(float) + 15u) & ~(size_t)15u, nbytes = info.with_normals ? vbytes : 0;
    MeshStage st;
    rc = stage_mesh_update(c, in_bytes, in_bytes + vbytes + nbytes, st);
    if (rc != JPT_OK) return rc;
    if (pbytes) std::memcpy(st.h + head, bone_transforms12, pbytes);
    std::memset(st.h + head + pbytes, 0, abytes);
    if (!active.empty()) std::memcpy(st.h + head + pbytes, active.data(), active.size() * sizeof(SkinShape));
    // d_mesh_in is read and written by work on the refit stream alone (the copies and kernels of the updates and poses; no render, read-back or
    // instance refit touches it), and that stream runs in order: the pose's copy and the skin kernel are queued AHEAD of the drain wait,
    // so they run beside the renders still in flight; only the refit of the shared records waits for them.
    char* in = c->upd.d_mesh_in.p;
    HIP_TRY(c, hipMemcpyAsync(in, st.h, in_bytes, hipMemcpyHostToDevice, c->upd.refit_stream));
    SkinArgs a;
    a.rig = skin_rig_view(info, rig.d_rig.p);
    a.influences = info.influences;
    a.palette = reinterpret_cast<const float*>(in + head);
    a.n_bones = n_pal;
    a.active = reinterpret_cast<const SkinShape*>(in + head + pbytes);
    a.n_active = (uint32_t)active.size();
    a.verts_out = reinterpret_cast<float*>(in + in_bytes);
    a.normals_out = info.with_normals ? reinterpret_cast<float*>(in + in_bytes + vbytes) : nullptr;
    launch_mesh_skin(c->upd.refit_stream, a);
    HIP_TRY(c, hipGetLastError());
    // The BLAS records, triangle records and root boxes are shared by every copy of the instance level: one pipeline drain on the
    // device, as jpt_scene_update_mesh
    HIP_TRY(c, drain_pipeline(c));
    return queue_mesh_refit(c, mesh_id, rebuild, a.verts_out, a.normals_out, reinterpret_cast<const float*>(st.dev + in_bytes), st, t0);
}

}  // namespace

int jpt_scene_pose_mesh(jpt_ctx* c, uint32_t mesh_id, const float* bone_transforms12, uint32_t n_bones, const float* blend_weights, uint32_t n_blend_weights)
{
    return pose_mesh(c, mesh_id, bone_transforms12, n_bones, blend_weights, n_blend_weights, false, "jpt_scene_pose_mesh");
}
int jpt_scene_pose_mesh_rebuild(jpt_ctx* c, uint32_t mesh_id, const float* bone_transforms12, uint32_t n_bones, const float* blend_weights, uint32_t n_blend_weights)
{
    return pose_mesh(c, mesh_id, bone_transforms12, n_bones, blend_weights, n_blend_weights, true, "jpt_scene_pose_mesh_rebuild");
}

int jpt_debug_mesh_records(jpt_ctx* c, uint32_t mesh_id, void* nodes4_out, void* nodesq_out, uint32_t node_capacity, void* tris_out,
                           void* shade_out, uint32_t tri_capacity, int32_t* info_out)
{
    if (!c || !info_out) return JPT_E_INVALID;
    if (const int rc = needs_scene(c, kWatertightTree, "jpt_debug_mesh_records", " needs a scene committed with JPT_BUILD_SAH_WATERTIGHT"); rc != JPT_OK) return rc;
    if (mesh_id >= c->scene.builder.mesh_count()) return fail(c, JPT_E_INVALID, "no such mesh");
    int rc = on_device(c, "host-only context: the records are on the device", false);
    if (rc == JPT_OK) rc = ensure_mesh_refit(c);
    if (rc != JPT_OK) return rc;
    const SceneUpdates::MeshRefit& mr = c->upd.mesh_refit[mesh_id];
    const int32_t info[6] = {mr.has_tree ? 1 : 0, mr.root4, (int32_t)mr.rec_first, (int32_t)mr.n_recs, (int32_t)mr.tri_first, (int32_t)mr.n_tris};
    std::memcpy(info_out, info, sizeof info);
    if (!mr.has_tree) return JPT_OK;
    if ((nodes4_out || nodesq_out) && node_capacity < mr.n_recs) return fail(c, JPT_E_INVALID, "record buffers too small");
    if ((tris_out || shade_out) && tri_capacity < mr.n_tris) return fail(c, JPT_E_INVALID, "triangle buffers too small");
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the context's stream follows every update)
    if (nodes4_out && mr.n_recs)
        HIP_TRY(c, hipMemcpy(nodes4_out, c->dev.nodes4.p + mr.rec_first, (size_t)mr.n_recs * sizeof(WideNode4), hipMemcpyDeviceToHost));
    if (nodesq_out && mr.n_recs)
        HIP_TRY(c, hipMemcpy(nodesq_out, c->dev.nodesq.p + mr.rec_first, (size_t)mr.n_recs * sizeof(WideNodeQ), hipMemcpyDeviceToHost));
    if (tris_out) HIP_TRY(c, hipMemcpy(tris_out, c->dev.wtris.p + mr.tri_first, (size_t)mr.n_tris * sizeof(WideTri), hipMemcpyDeviceToHost));
    if (shade_out) HIP_TRY(c, hipMemcpy(shade_out, c->dev.shade_tris.p + mr.tri_first, (size_t)mr.n_tris * sizeof(ShadeTri), hipMemcpyDeviceToHost));
    return JPT_OK;
}

int jpt_debug_tlas_records(jpt_ctx* c, void* nodes4_out, void* nodesq_out, uint32_t capacity, uint32_t* n_records, int32_t* root_out, float* inst_lo3,
                           float* inst_hi3)
{
    if (const int rc = needs_scene(c, kNativeTree, "jpt_debug_tlas_records", " needs a scene made by jpt_scene_commit with the native builder"); rc != JPT_OK) return rc;
    if (const int rc = on_device(c, "host-only context: the records are on the device", true); rc != JPT_OK) return rc;
    const size_t nt = c->scene.wide.tlas_nodes4.size(), ni = c->scene.ref.instances.size();
    const int32_t base = (int32_t)c->upd.tail_first(c->scene.wide, c->upd.cur_set);
    if (n_records) *n_records = (uint32_t)nt;
    if (root_out) *root_out = c->ds.tlas_root4 >= 0 ? c->ds.tlas_root4 - base : c->ds.tlas_root4;
    if ((nodes4_out || nodesq_out) && capacity < nt) return fail(c, JPT_E_INVALID, "record buffers too small");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the context's stream follows every refit)
    if (nodes4_out && nt) {
        HIP_TRY(c, hipMemcpy(nodes4_out, c->dev.nodes4.p + base, nt * sizeof(WideNode4), hipMemcpyDeviceToHost));
        WideNode4* r = static_cast<WideNode4*>(nodes4_out);
        for (size_t i = 0; i < nt; i++)
            for (int k = 0; k < 4; k++)
                if (r[i].child[k] >= 0) r[i].child[k] -= base;
    }
    if (nodesq_out && nt) {
        HIP_TRY(c, hipMemcpy(nodesq_out, c->dev.nodesq.p + base, nt * sizeof(WideNodeQ), hipMemcpyDeviceToHost));
        WideNodeQ* r = static_cast<WideNodeQ*>(nodesq_out);
        for (size_t i = 0; i < nt; i++)
            for (int k = 0; k < 4; k++)
                if (r[i].child[k] >= 0) r[i].child[k] -= base;
    }
    if ((inst_lo3 || inst_hi3) && ni) {
        std::vector<RefInstance> inst(ni);
        HIP_TRY(c, hipMemcpy(inst.data(), c->dev.set[c->upd.cur_set].inst.p, ni * sizeof(RefInstance), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ni; i++) {
            if (inst_lo3) inst_lo3[3 * i] = inst[i].aabbMin.x, inst_lo3[3 * i + 1] = inst[i].aabbMin.y, inst_lo3[3 * i + 2] = inst[i].aabbMin.z;
            if (inst_hi3) inst_hi3[3 * i] = inst[i].aabbMax.x, inst_hi3[3 * i + 1] = inst[i].aabbMax.y, inst_hi3[3 * i + 2] = inst[i].aabbMax.z;
        }
    }
    return JPT_OK;
}
