// jpt_render.cpp -- how a render is planned, launched, pipelined and timed (RenderPipe, jpt_ctx.h): the three render entry points and what
// they are made of -- validate, prepare, plan (plan_launch: every measured scheduling rule, with the measurements), launch, read back -- the
// pipeline slots and the frame groups' helper streams, the policy calls that shape them (jpt_set_stream_priority, jpt_set_memory_policy,
// jpt_get_workspace_bytes, jpt_renders_in_flight, jpt_set_kernel_timing), jpt_sync, and the temporal pass's parameters (jpt_set_temporal_params) and part of a render (TemporalState).
#include "jpt_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jpt_tuning.h"

hipError_t RenderPipe::create_events()
{
    const hipError_t e = hipEventCreate(&ev0);
    return e != hipSuccess ? e : hipEventCreate(&ev1);
}

hipError_t RenderPipe::drain_slots()
{
    for (const PipeSlot& ps : slot)
        if (ps.stream)
            if (const hipError_t e = hipStreamSynchronize(ps.stream); e != hipSuccess) return e;
    return hipSuccess;
}

// drain and destroy the pipeline slots' streams and the frame groups' helper streams (a borrowed helper is a slot's stream: it
// goes with the slot); the next render that needs them makes new ones
void RenderPipe::release_streams()
{
    for (int k = 0; k < kMaxGroups - 1; k++) {
        hipStream_t& st = group_streams.aux_stream[k];
        if (st) {
            (void)hipStreamSynchronize(st);
            if (!aux_borrowed[k]) (void)hipStreamDestroy(st);
        }
        st = nullptr;
        aux_borrowed[k] = false;
    }
    for (PipeSlot& ps : slot) {
        if (ps.stream) {
            (void)hipStreamSynchronize(ps.stream);
            (void)hipStreamDestroy(ps.stream);
        }
        ps.stream = nullptr;
        ps.acc_done_valid = false;
    }
}

void RenderPipe::destroy()
{
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (hipEvent_t e : trace_events) (void)hipEventDestroy(e);
    release_streams();
    for (hipEvent_t e : group_streams.join) if (e) (void)hipEventDestroy(e);
    if (group_streams.fork) (void)hipEventDestroy(group_streams.fork);
    for (PipeSlot& ps : slot) {
        if (ps.ev_paths_done) (void)hipEventDestroy(ps.ev_paths_done);
        if (ps.ev_acc_done) (void)hipEventDestroy(ps.ev_acc_done);
    }
}

namespace {

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
    const WideScene& w = c->scene.wide;
    const bool use4 = c->scene.walks_nodes4();
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
    const size_t budget = c->pipe.workspace_budget ? (size_t)c->pipe.workspace_budget : (size_t)tuning().workspace_budget_mb << 20;
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
    if (c->device < 0 || !c->scene.device_ready || !c->params_set || !c->camera_set || n_frames <= 0)
        return do_render_batch(c, n_frames, first_frame_index, counted, blocking);  // reports the error / no-op
    // a budget the caller set is a cap, not a hint: one frame is the smallest batch there is
    if (c->pipe.workspace_budget && c->kernel_variant != JPT_KERNEL_REFERENCE_LAYOUT && !c->debug_steps) {
        const size_t one = wf2_workspace_bytes(c->width, c->local_rows, 1, c->max_bounces, lighting_bound(c));
        if (one > c->pipe.workspace_budget)
            return fail(c, JPT_E_LIMIT, "jpt_set_memory_policy: one frame of this resolution needs a workspace of " + std::to_string(one) +
                                            " bytes, the budget is " + std::to_string(c->pipe.workspace_budget) +
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
    Wf2Streams& gs = c->pipe.group_streams;
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
            const bool borrow = c->pipe.slot_priority != JPT_STREAM_PRIORITY_NORMAL && c->pipe.slot_priority != JPT_STREAM_PRIORITY_LOW;
            if (borrow) {
                if (!ensure_pipe_slot(c, k)) break;
                gs.aux_stream[k] = c->pipe.slot[k].stream;
                c->pipe.aux_borrowed[k] = true;
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
    PipeSlot& ps = c->pipe.slot[k];
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
        const bool normal = c->pipe.slot_priority == JPT_STREAM_PRIORITY_NORMAL, low = c->pipe.slot_priority == JPT_STREAM_PRIORITY_LOW;
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
    if (c->pipe.six_queues >= 0) return c->pipe.six_queues != 0;
    c->pipe.six_queues = 0;
    constexpr int kProbe = 6;
    for (int k = 0; k < kProbe; k++)
        if (!ensure_pipe_slot(c, k)) return false;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        return false;
    }
    const long long ticks = (long long)khz * 400 / 1000;   // 0.4 ms
    for (int k = 0; k < kProbe; k++) launch_queue_spin(c->pipe.slot[k].stream, 1);   // (the module is loaded, the queues exist)
    for (int k = 0; k < kProbe; k++)
        if (hipStreamSynchronize(c->pipe.slot[k].stream) != hipSuccess) return false;
    double best = 1e9;
    for (int rep = 0; rep < 2; rep++) {   // the better of two: a host hiccup can only make it look serial
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < kProbe; k++) launch_queue_spin(c->pipe.slot[k].stream, ticks);
        for (int k = 0; k < kProbe; k++)
            if (hipStreamSynchronize(c->pipe.slot[k].stream) != hipSuccess) return false;
        best = std::min(best, ms_since(t0));
    }
    if (hipGetLastError() != hipSuccess) return false;
    c->pipe.six_queues = best < 0.4 * 1.6 ? 1 : 0;
    return c->pipe.six_queues != 0;
}

// the event the last render left on the context's stream has completed: nothing of this context is in flight
bool pipeline_idle(jpt_ctx* c)
{
    const bool idle = hipEventQuery(c->pipe.ev1) == hipSuccess;
    (void)hipGetLastError();   // (hipErrorNotReady is an answer, not an error)
    return idle;
}

const PlanDevice kPlanDevice{six_queues_probe, pipeline_idle, ensure_pipe_slot, ensure_group_streams};

}  // namespace

// Every rule of a render's launch shape, in one place.  Makes no HIP call of its own; keeps c->pipe.last_pipe_slots and
// c->pipe.idle_streak.  fp: the render's frame_params; r: its sky cull and lighting.
LaunchPlan jpt::plan_launch(jpt_ctx* c, const FrameParams& fp, const Wf2Render& r, bool counted, bool blocking, const PlanDevice& dev)
{
    LaunchPlan p;
    if (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps) return p;   // (DEBUG_STEPS exists in the audit kernel only)
    const bool timed = c->kernel_timing;   // per-launch events want the launches of a render one after another
    // renders in flight (JPT_PIPE_SLOTS overrides): a render is eleven dependent launches of >= 25-30 us each
    // however little work it holds, so several of them are needed to fill the chip
    const int env_slots = tuning().pipe_slots;   // (after the embedding application's cap, jpt_set_memory_policy)
    const int forced_slots = c->pipe.max_slots > 0 ? c->pipe.max_slots : (env_slots <= 0 ? 0 : std::min(std::max(env_slots, 2), (int)RenderPipe::kPipeSlots));
    // Four renders in flight, each tracing with a quarter of the blocks (four consecutive segments per block: a
    // deeper queue keeps a block's lanes refilled for a larger share of its launch) beat two renders of full-width
    // launches on every size tried: C3 1.32 vs 1.45 ms, C2 0.36 vs 0.46, 1 frame 0.30 vs 0.37, 1920x136 0.185 vs
    // 0.193, 4K x 16 spp 11.1 vs 11.1.  Renders whose workspace exceeds 24 GiB keep two slots and full-width launches
    // (4 x 24 GiB of workspaces is where this stops).
    const bool huge = wf2_workspace_bytes(c->width, c->local_rows, fp.n_frames, c->max_bounces, r.lighting) > ((size_t)24 << 30);
    // ... six where the slots' streams have six hardware queues to themselves (six_queues_probe), four otherwise
    const bool may_queue = tuning().pipelining && !blocking && !counted;
    const int slots = forced_slots ? forced_slots : (huge ? 2 : ((may_queue && dev.six_queues(c)) ? 6 : 4));
    if (may_queue) c->pipe.last_pipe_slots = slots;
    // A host that queues ONE render at a time (jpt_render_async, its own work, jpt_sync or the split read-back, again)
    // never has a second render in flight: the pipelined form's quarter-width launches then run alone, and a render takes
    // half as long again as a blocking one (C3 1.93 against 1.26 ms, 3840 x 2160 x 4 spp 3.33 against 2.11:
    // tools/lone_async_probe.py).  The third queued render in a row that finds nothing in flight -- the event every render
    // leaves on the context's stream has completed -- is launched like a blocking one instead (frame groups, full-width
    // launches; nobody waits for it here), and so on until a render finds work in flight.  A queue of renders is not
    // affected: only its first render finds the pipeline empty.
    bool lone = false;
    if (may_queue && !timed) {
        c->pipe.idle_streak = dev.idle(c) ? c->pipe.idle_streak + 1 : 0;
        lone = c->pipe.idle_streak >= 3;
    }
    const int slot = (int)(c->pipe.async_seq % (uint64_t)slots);
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
    const size_t walked_bytes = c->scene.wide.blas_nodes4.size() * sizeof(WideNodeQ) + c->scene.wide.tris.size() * sizeof(WideTri);
    const bool small = window_paths <= 1500000u && walked_bytes <= ((size_t)32 << 20);
    p.chain = (p.groups == 2 || (c->scene.walks_nodes4() && small)) ? 2 : 1;
    return p;
}

namespace {

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
    for (int32_t k = 0; k + 1 < c->pipe.trace_events_used; k += 2) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, c->pipe.trace_events[(size_t)k], c->pipe.trace_events[(size_t)k + 1]) == hipSuccess) {
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
    if (!c->scene.device_ready) return fail(c, JPT_E_STATE, "no scene: call jpt_scene_upload_reference_layout or jpt_scene_commit first");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    if (!c->camera_set) return fail(c, JPT_E_STATE, "jpt_set_camera not called");
    if (n_frames < 0) return fail(c, JPT_E_INVALID, "n_frames < 0");
    if (c->upd.mesh_deformed && (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps))
        return fail(c, JPT_E_STATE, "jpt_scene_update_mesh refits the default kernel's records only: call jpt_scene_commit before rendering with another kernel");
    if (c->upd.refit_active && (c->kernel_variant != JPT_KERNEL_WAVEFRONT || c->debug_steps))
        return fail(c, JPT_E_STATE, "jpt_scene_refit_tlas refits the default kernel's records only: call jpt_scene_update_tlas before rendering with another kernel");
    return JPT_OK;
}

// What a render needs before it is planned (after prepare_temporal): zeroed counters, the workspace of the context's
// stream, the timing events, and (wavefront renders) the sky cull and the tiles' sky cells in r.  r.lighting and r.primary are the render's.
int prepare_render(jpt_ctx* c, const FrameParams& fp, bool counted, bool wavefront, Wf2Render& r)
{
    hipStream_t s = c->stream;
    const int32_t n_frames = fp.n_frames;
    if (counted) HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(DevCounters), s));
    const bool wf2 = wavefront && c->local_rows > 0 && c->width > 0 && n_frames > 0;
    if (wf2) {
        const size_t need = wf2_workspace_bytes(c->width, c->local_rows, n_frames, c->max_bounces, r.lighting);
        if (c->pipe.slot[0].workspace.n < need) {
            HIP_TRY(c, hipStreamSynchronize(s));
            HIP_TRY(c, c->pipe.slot[0].workspace.resize(need));
        }
    }
    HIP_TRY(c, hipEventRecord(c->pipe.ev0, s));
    if (!wf2) return JPT_OK;
    const size_t need_ev = c->kernel_timing ? 2 * (size_t)(c->max_bounces + 1) : 0;
    while (c->pipe.trace_events.size() < need_ev) {
        hipEvent_t e;
        HIP_TRY(c, hipEventCreate(&e));
        c->pipe.trace_events.push_back(e);
    }
    c->pipe.trace_events_used = (int32_t)need_ev;
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
        if (!c->pipe.sky_tiles_valid || c->pipe.d_sky_tiles.n < n_tiles || std::memcmp(key, c->pipe.sky_tiles_key, sizeof key) != 0 ||
            std::memcmp(&cam_key, &c->pipe.sky_tiles_camera, sizeof cam_key) != 0) {
            if (c->pipe.d_sky_tiles.n < n_tiles) {
                HIP_TRY(c, hipStreamSynchronize(s));   // (renders in flight may read the old buffer)
                if (const hipError_t e = c->pipe.drain_slots(); e != hipSuccess) return hip_fail(c, e, "hipStreamSynchronize(ps.stream)");
                HIP_TRY(c, c->pipe.d_sky_tiles.resize(n_tiles));
            }
            launch_sky_tiles(s, fp, c->camera, c->pipe.d_sky_tiles.p);
            std::memcpy(c->pipe.sky_tiles_key, key, sizeof key);
            c->pipe.sky_tiles_camera = cam_key;
            c->pipe.sky_tiles_valid = true;
        }
        r.sky_tiles = c->pipe.d_sky_tiles.p;
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
            launch_ref_frame(s, c->ds, one, c->camera, c->image.d_accum.p, c->image.d_ldr.p, depth_img, cnt, r.lighting, r.primary);
        }
        return JPT_OK;
    }
    if (p.route == LaunchPlan::kStream) {
        launch_wf2_render(s, c->ds, fp, c->camera, c->pipe.slot[0].workspace.p, c->image.d_accum.p, c->image.d_ldr.p, depth_img, cnt,
                          c->kernel_timing ? c->pipe.trace_events.data() : nullptr, r, p.groups, p.chain, c->pipe.group_streams);
        return JPT_OK;
    }
    // a queued render: path kernels and accumulation on the slot's stream with the slot's workspace
    PipeSlot& ps = c->pipe.slot[p.slot];
    const size_t need = wf2_workspace_bytes(c->width, c->local_rows, fp.n_frames, c->max_bounces, r.lighting);
    bool slots_ready = true;
    for (int k = 0; k < p.slots; k++) slots_ready = slots_ready && c->pipe.slot[k].stream && c->pipe.slot[k].workspace.n >= need;
    if (!slots_ready) {
        // The first queued render of this size prepares ALL the slots, so that none of it lands in the middle
        // of a queue of renders: a stream that gets its own hardware queue costs ~6 ms to create, a device
        // allocation waits for the device, and a fresh 2 GB allocation costs its first user ~10 ms.
        HIP_TRY(c, hipStreamSynchronize(s));  // every earlier render ends with a kernel on `s`
        for (int k = 0; k < p.slots; k++) {
            PipeSlot& sk = c->pipe.slot[k];
            if (sk.workspace.n < need) {
                HIP_TRY(c, sk.workspace.resize(need));
                HIP_TRY(c, hipMemsetAsync(sk.workspace.p, 0, need, s));  // first touch
                c->pipe.workspace_touched(k);
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
    launch_wf2_render(ps.stream, c->ds, fp, c->camera, ps.workspace.p, c->image.d_accum.p, c->image.d_ldr.p, depth_img, nullptr, nullptr, r,
                      p.groups, p.chain, c->pipe.group_streams);
    HIP_TRY(c, hipEventRecord(ps.ev_acc_done, ps.stream));
    HIP_TRY(c, hipStreamWaitEvent(s, ps.ev_acc_done, 0));
    ps.acc_done_valid = true;
    c->pipe.async_seq++;
    return JPT_OK;
}

// a blocking or counted render: its time, ray count and event counters
int read_back_stats(jpt_ctx* c, const FrameParams& fp, bool counted, bool wavefront, const SkyCull& cull)
{
    HIP_TRY(c, hipEventSynchronize(c->pipe.ev1));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->pipe.ev0, c->pipe.ev1));
    c->stats.last_render_ms = ms;
    c->stats.last_trace_ms = ms;
    if (wavefront && c->pipe.trace_events_used > 0 && fp.n_frames > 0 && c->local_rows > 0) c->stats.last_trace_ms = traced_ms(c, &c->stats.last_primary_ms);
    if (wavefront && c->pipe.slot[0].workspace.p && fp.n_frames > 0 && c->local_rows > 0) {
        // ray segments traced = sum of the per-bounce queue sizes (always available on this route)
        const size_t nq = (size_t)c->max_bounces + 2, per_row = wf2_segments();
        c->pipe.h_qcount.assign(nq * per_row + 2u, 0u);   // queue sizes, then the set-aside counts
        HIP_TRY(c, hipMemcpy(c->pipe.h_qcount.data(), c->pipe.slot[0].workspace.p, c->pipe.h_qcount.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        c->stats.set_aside = c->pipe.h_qcount[nq * per_row];
        c->stats.set_aside_dropped = c->pipe.h_qcount[nq * per_row + 1u];
        // every in-image (pixel, frame) has one primary segment; rows 1.. hold the later bounces' queue sizes
        uint64_t rays = (uint64_t)c->width * (uint64_t)c->local_rows * (uint64_t)fp.n_frames;
        for (int b = 1; b <= c->max_bounces; b++)
            for (size_t k = 0; k < per_row; k++) rays += c->pipe.h_qcount[(size_t)b * per_row + k];
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

// What the temporal pass needs before its render is prepared: its four refusals, and zero-filled history images when it starts over
int prepare_temporal(jpt_ctx* c, int32_t n_frames)
{
    if (c->denoise != JPT_DENOISE_TEMPORAL) return JPT_OK;
    hipStream_t s = c->stream;
    // the pass runs once per displayed frame and reads other pixels' depth and history (temporal_reprojection.glsl:57-61)
    if (n_frames > 1) return fail(c, JPT_E_INVALID, "temporal reprojection renders one frame per call");
    if (c->world != 1) return fail(c, JPT_E_STATE, "temporal reprojection needs the whole image in one context (world == 1)");
    if (!c->reproj.temporal_set) return fail(c, JPT_E_STATE, "jpt_set_temporal_params not called");
    if (c->reproj.temporal.width != c->width || c->reproj.temporal.height != c->height)
        return fail(c, JPT_E_INVALID, "temporal RenderParameters width/height differ from jpt_set_params");
    const size_t npx = (size_t)c->width * c->height;
    if (!c->reproj.hist_valid || c->reproj.d_hist1.n != npx) {
        // Image::create(...) zero-filled history images (temporal_reprojection.cpp:42-43)
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, c->reproj.d_hist1.resize(npx));
        HIP_TRY(c, c->reproj.d_hist2.resize(npx));
        if (npx) {
            HIP_TRY(c, hipMemsetAsync(c->reproj.d_hist1.p, 0, npx * sizeof(float4), s));
            HIP_TRY(c, hipMemsetAsync(c->reproj.d_hist2.p, 0, npx * sizeof(float4), s));
        }
        c->reproj.hist_valid = true;
        c->reproj.hist_written = nullptr;
    }
    return JPT_OK;
}

// validate -> prepare -> plan -> launch -> read back
int do_render_batch(jpt_ctx* c, int32_t n_frames, uint32_t first_frame_index, bool counted, bool blocking)
{
    int rc = validate_render(c, n_frames);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    restart_sum(c, kSumRendered);   // (an assembled image is of the frames before this render)
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
    if ((rc = prepare_temporal(c, n_frames)) != JPT_OK) return rc;
    if ((rc = prepare_render(c, fp, counted, wavefront, r)) != JPT_OK) return rc;
    bool pipelined = false;
    if (c->local_rows > 0 && c->width > 0 && n_frames > 0) {
        c->image.depth_valid = want_depth;
        const LaunchPlan p = plan_launch(c, fp, r, counted, blocking, kPlanDevice);
        rc = launch_render(c, p, fp, r, counted ? c->d_counters.p : nullptr, want_depth ? c->image.d_depth.p : nullptr);
        if (rc != JPT_OK) return rc;
        if (r.bake_dir) c->post.bake_dir_valid = true;
        if (r.variance) c->post.variance_valid = true;
        pipelined = p.route == LaunchPlan::kSlot;
        if (c->denoise == JPT_DENOISE_TEMPORAL) {
            // TemporalReprojection::render's dispatch (temporal_reprojection.cpp:71): screen + depth of this frame in,
            // blended history and the displayed screen out
            launch_temporal(c->stream, c->reproj.temporal, c->image.d_ldr.p, c->image.d_depth.p, c->reproj.d_hist1.p, c->reproj.d_hist2.p);
            c->reproj.hist_written = (c->reproj.temporal.frame_count % 2u) == 0u ? c->reproj.d_hist2.p : c->reproj.d_hist1.p;
        }
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->pipe.ev1, c->stream));
    if (wavefront && !pipelined) c->pipe.workspace_touched(0);  // slot 0's workspace was used on the context's stream itself
    c->frame_count += (uint32_t)n_frames;
    c->stats.frames = c->frame_count;
    return (blocking || counted) ? read_back_stats(c, fp, counted, wavefront, r.cull) : JPT_OK;
}

}  // namespace

extern "C" {

int jpt_renders_in_flight(const jpt_ctx* c) { return c ? c->pipe.last_pipe_slots : 0; }

int jpt_set_stream_priority(jpt_ctx* c, int32_t priority)
{
    if (!c) return JPT_E_INVALID;
    if (priority < JPT_STREAM_PRIORITY_DEFAULT || priority > JPT_STREAM_PRIORITY_LOW) return fail(c, JPT_E_INVALID, "unknown stream priority");
    if (priority == c->pipe.slot_priority) return JPT_OK;
    c->pipe.slot_priority = priority;
    if (c->device < 0) return JPT_OK;
    // the pipeline slots' streams are made on first use: drop the ones that exist, the next queued render makes new ones
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->pipe.release_streams();   // (the frame groups' helper streams follow them)
    c->pipe.six_queues = -1;   // (measured again for the new streams)
    return JPT_OK;
}

int jpt_set_memory_policy(jpt_ctx* c, int32_t renders_in_flight, uint64_t workspace_budget_bytes)
{
    if (!c) return JPT_E_INVALID;
    if (renders_in_flight < 0 || renders_in_flight > RenderPipe::kPipeSlots) return fail(c, JPT_E_INVALID, "renders_in_flight must be 0 (the library's rule) or 1..8");
    c->pipe.max_slots = renders_in_flight;
    c->pipe.workspace_budget = workspace_budget_bytes;
    if (c->device < 0) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // drain, then give back what the new policy no longer allows: the workspaces of slots past the cap, and any workspace
    // larger than the new budget (the next render allocates what it needs)
    if (const hipError_t e = c->pipe.drain_slots(); e != hipSuccess) return hip_fail(c, e, "hipStreamSynchronize(ps.stream)");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int keep = renders_in_flight > 0 ? renders_in_flight : RenderPipe::kPipeSlots;
    for (int k = 0; k < RenderPipe::kPipeSlots; k++) {
        PipeSlot& ps = c->pipe.slot[k];
        if (k >= keep || (workspace_budget_bytes && ps.workspace.n > workspace_budget_bytes)) {
            ps.workspace.release();
            c->pipe.workspace_touched(k);
        }
    }
    c->pipe.async_seq = 0;   // the next queued render starts at slot 0 again
    release_read_staging(c);   // (the pinned staging of the blocking read-backs: re-made by the next one)
    return JPT_OK;
}

int jpt_get_workspace_bytes(jpt_ctx* c, uint64_t* bytes_out)
{
    if (!c || !bytes_out) return JPT_E_INVALID;
    uint64_t n = 0;
    for (const PipeSlot& ps : c->pipe.slot) n += ps.workspace.n;
    *bytes_out = n;
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
    if (hipEventElapsedTime(&ms, c->pipe.ev0, c->pipe.ev1) == hipSuccess) c->stats.last_render_ms = c->stats.last_trace_ms = ms;
    else (void)hipGetLastError();   // (no render recorded yet -- queries alone: not an error to leave behind for the host's next HIP call)
    if (c->kernel_variant != JPT_KERNEL_REFERENCE_LAYOUT && c->pipe.trace_events_used > 0) c->stats.last_trace_ms = traced_ms(c, nullptr);
    return JPT_OK;
}

int jpt_set_kernel_timing(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    c->kernel_timing = enable != 0;
    if (!c->kernel_timing) c->pipe.trace_events_used = 0;
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

}  // extern "C"
