// jpt_kernels_wf2.hip -- the native (fast) route: persistent-block wavefront path tracer.
//
// All `n_frames` frames of a render are in flight at once as independent paths (pixel x frame); per-pixel
// RNG streams (main.glsl:409, :386) are carried with the path, so the schedule cannot change results.
// The grid is G persistent blocks.  Block s owns SEGMENT s of every queue: chunks of 64 consecutive path ids
// (path = pixel slot * n_frames + frame: every frame's sample of a few neighbouring pixels of an 8x8 tile)
// are dealt round-robin to segments, so each segment is a uniform sample of the image and all hand-offs
// between kernels stay inside a segment -- no global atomics anywhere on the path.
//
//   wf2_primary  bounce 0: generates primary rays (main.glsl:405-421) and traces them.  Sky misses are
//                finished on the spot; hits are packed into the segment's queue (LDS counter).
//   wf2_shade    one path vertex per queue entry (main.glsl:378-397 + brdfs.glsl); survivors' next rays are
//                packed to the front of the segment's next queue (wave ballot + prefix popcount + LDS base).
//   wf2_trace    bounces >= 1: closest hit of every queued ray.
//   wf2_finish   the few paths wf2_shade set aside (hits the reference's traversal cannot reach, exact distance ties).
//   wf2_accumulate  frames IN ORDER per pixel (progressive_rendering.glsl:33-37), display image, depth.
//   (large scenes: the tracing kernels' TAIL instantiations finish their few very long walks with a whole wave per ray,
//   coop_walk_call)
// wf2_primary, wf2_shade, wf2_finish and wf2_accumulate see the paths' misses: they live in jpt_wf2_paths.h, included twice --
// as themselves, and as the *_env kernels that light the misses with an environment map (jpt_set_environment).
//
// Tracing kernels keep every lane busy: a lane whose ray is finished takes the next ray of the block's
// segment (cursor in LDS) while its neighbours keep walking -- the wave never waits for its slowest ray.
// Per-lane traversal stacks live in LDS (20 entries x 256 lanes, deeper levels spill to scratch).
//
// launch_wf2_render runs one render in the frame groups (this pipeline on several streams at once) and with the tracing
// chain the host chose; the host decides those, and pipelines asynchronous renders one level up (plan_launch, jpt_capi.cpp).
#include <algorithm>
#include <cstdlib>

#include "jpt_trace_core.h"
#include "jpt_tie_walk.h"
#include "jpt_tuning.h"
#include "jpt_variance.h"

// the primary kernel carries the ray set-up and the sky-cull test besides the walk: 74 VGPRs on its own.  Round 1 (float
// records) ran it at 6 waves/SIMD because 72 registers spilled; with the quantised records two registers are all the
// cap takes away and 7 waves/SIMD are 0.3-0.5 % ahead of 6 (four A/B repetitions, tools/ab_rates.sh); 5 are 1 % behind
#ifndef JPT_PRIMARY_WAVES
#define JPT_PRIMARY_WAVES 7
#endif

namespace jpt {

namespace {

constexpr int kBlock = kTraceBlock;
constexpr uint32_t kSegments = 256u * JPT_WAVES_PER_SIMD;  // persistent grid: one 256-thread block per CU per wave/SIMD
struct WfTune {
    int refill_idle;     // refill when at least this many lanes of a wave are idle
    int primary_refill_idle;   // ... in the primary launch
    int node_min_lanes;  // leave the node loop when fewer lanes than this still descend
    int leaf_min_lanes;  // a leaf / instance phase with fewer takers than this is put off to the next round, as long as
    int inst_min_lanes;  // other lanes of the wave can make progress meanwhile
    int phase_frac16;    // ... and never more than this many sixteenths of the wave's active rays
    int tail_rounds;     // TAIL launches: a wave enters its tail phase this many rounds after the queue ran dry ...
    int tail_lanes;      // ... once it holds at most this many rays
};

// One round of the walk for every active lane of the wave, "while-while" style so that lanes in different
// states do not serialise each other's code: (1) a tight loop of internal-record steps (lanes that reach a
// leaf wait), (2) triangle leaves, (3) instance entries.  Returns true for lanes whose walk is complete.
template <bool COUNT, bool W4>
__device__ __forceinline__ bool walk_round(Traversal<COUNT, W4>& tr, bool active, const WideSceneDev& sc,
                                           const typename Traversal<COUNT, W4>::Stack& st, DevCounters& cnt, const WfTune& tune, uint32_t& steps)
{
    const int kNodeMinLanes = tune.node_min_lanes;
    const bool lane0 = (threadIdx.x & 63) == 0;
    if (COUNT && lane0) cnt.phase[0]++;
    // A thinly attended leaf or instance phase waits for more takers while the wave has other work -- lanes that still
    // descend (the next round's record loop) or the other phase: a phase costs the wave the same whether 4 or 40 lanes take
    // part.  The thresholds shrink with the wave's rays (never more than phase_frac16 sixteenths of them): a wave that is
    // draining must not make its last rays wait.  C3 -3.5 %, close-up -5.5 %, C2 -3 % (tools/sweep_sched.sh: a plateau
    // from 8 to 32 lanes for leaves and 4 to 16 for instance entries at a quarter of the rays; without the cap small
    // renders lose 10 %).  Skipping a thinly attended record loop in the same way changes nothing.
    const int na = __popcll(__ballot(active));
    const int cap = (na * tune.phase_frac16) >> 4;
    const int lmin = tune.leaf_min_lanes < cap ? tune.leaf_min_lanes : cap;
    const int imin = tune.inst_min_lanes < cap ? tune.inst_min_lanes : cap;
    for (int it = 0; it < 64; it++) {
        if (active && !tr.have && tr.sp > 0) tr.pop_next(st);
        const bool want = active && tr.wants_node();
        const unsigned long long m = __ballot(want);
        if (m == 0 || (it > 0 && __popcll(m) < kNodeMinLanes)) break;
        if (COUNT && lane0) {
            cnt.phase[1]++;
            cnt.phase[2] += (unsigned long long)__popcll(m);
        }
        if (want) tr.node_step(sc, st, cnt);
        if (COUNT && want) steps++;
    }
    bool wl = active && tr.wants_leaf();
    bool wi = active && tr.wants_instance();
    if (W4 && (tune.leaf_min_lanes > 1 || tune.inst_min_lanes > 1)) {   // (reference trees, with leaves of up to 64 triangles, lose 5 % by waiting)
        const int nl = __popcll(__ballot(wl)), ni = __popcll(__ballot(wi));
        const bool nodes_left = __any(active && tr.wants_node()) || __any(active && !tr.have && tr.sp > 0);
        const bool run_l = nl >= lmin || !(nodes_left || ni >= imin);
        const bool run_i = ni >= imin || !(nodes_left || (run_l && nl > 0));
        wl = wl && run_l;
        wi = wi && run_i;
    }
    if (COUNT) {
        const int nl = __popcll(__ballot(wl)), ni = __popcll(__ballot(wi));
        if (lane0 && nl) {
            cnt.phase[3]++;
            cnt.phase[4] += (unsigned long long)nl;
        }
        if (lane0 && ni) {
            cnt.phase[5]++;
            cnt.phase[6] += (unsigned long long)ni;
        }
    }
    if (wl) tr.leaf_step(sc, cnt);
    if (wi) tr.instance_step(sc, st, cnt);
    if (COUNT && (wl || wi)) steps++;
    return active && tr.finished();
}

// A lane mask as a per-lane predicate: costs nothing (the mask IS the predicate's register form).
__device__ __forceinline__ bool in_mask(const unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// The same round for the tracing launches (trace_queue), with the wave's bookkeeping on the SCALAR side.  `act` is the wave-uniform
// mask of the lanes that hold a ray; the round returns the mask of the lanes whose walk it completed.  Same steps per ray, same
// phase decisions and counters as walk_round; what differs is how the wave arrives at them:
//  - a ballot of a loop-carried flag, or of a conjunction, compiles to v_cndmask 0/1 + v_cmp_ne (2 x 4.2 cycles of VALU issue),
//    a ballot of ONE comparison to the comparison alone.  So nothing but single comparisons is balloted: cur < 0, cur >= 0,
//    cur == kSentinel, top > base, k0 < kNoChild; everything else is scalar and / andn2 / or on masks;
//  - `active` is not balloted at all: it is `act`, and the per-lane predicates come back from masks (in_mask);
//  - the walk's flags `have` and `in_blas` are not per-lane values but the two wave-uniform masks of WalkMasks, carried by
//    trace_queue from round to round.  Every update is made in wave-uniform control flow, from the mask of the branch the
//    lanes' step ran under: a pop sets the popping lanes' `have` (but for a sentinel that was the last entry), a sentinel clears
//    their `in_blas`, a record step leaves have = ballot(k0 < kNoChild) for its takers, a leaf step clears `have`, an instance
//    entry sets both, a refill sets `have` from n_instances != 0 and clears `in_blas` (trace_queue);
//  - the stack position is the LDS address of the lane's next entry (Traversal::Masked::top), sp > 0 is top > base;
//  - pop_next is written out here in two pieces, the pop and what follows a sentinel, each under the mask of its takers, with
//    the world ray's slab constants restored on demand (Traversal::restore_world: pop_next<true>'s restore), not once per round
//    in the loop's pre-header.
struct WalkMasks {
    unsigned long long have = 0ull, in_blas = 0ull;
};
template <bool COUNT, bool W4>
__device__ __forceinline__ unsigned long long walk_round_masked(Traversal<COUNT, W4>& tr, typename Traversal<COUNT, W4>::Masked& ml, WalkMasks& wm,
                                                                const unsigned long long act, const WideSceneDev& sc,
                                                                const typename Traversal<COUNT, W4>::Stack& st, DevCounters& cnt, const WfTune& tune,
                                                                uint32_t& steps)
{
    using Walk = Traversal<COUNT, W4>;
    const int kNodeMinLanes = tune.node_min_lanes;
    const bool lane0 = (threadIdx.x & 63) == 0;
    if (COUNT && lane0) cnt.phase[0]++;
    const int na = __popcll(act);
    const int cap = (na * tune.phase_frac16) >> 4;   // (the thresholds' caps: see walk_round)
    const int lmin = tune.leaf_min_lanes < cap ? tune.leaf_min_lanes : cap;
    const int imin = tune.inst_min_lanes < cap ? tune.inst_min_lanes : cap;
    const uint32_t base = Walk::lds_base(st);
    unsigned long long have_m = wm.have, blas_m = wm.in_blas;
    for (int it = 0; it < 64; it++) {
        // pop_next for the lanes that hold no record and have entries left (active && !have && sp > 0)
        const unsigned long long pm = act & ~have_m & __ballot(ml.top > base);
        if (pm) {
            if (in_mask(pm)) tr.cur = tr.pop_at(st, ml.top);
            const unsigned long long sent = pm & __ballot(tr.cur == kSentinel);
            have_m |= pm & ~sent;
            if (sent) {
                // out of the instance; if the sentinel was the last entry the walk is over (cur stays kSentinel, have false)
                blas_m &= ~sent;
                const unsigned long long more = sent & __ballot(ml.top > base);
                if (in_mask(more)) {
                    tr.cur = tr.pop_at(st, ml.top);
                    if (!Walk::kLean || tr.cur >= 0) tr.restore_world();   // (only a TLAS record reads the current-level ray: pop_next)
                }
                have_m |= more;
            }
        }
        const unsigned long long m = act & have_m & __ballot(tr.cur >= 0);   // wants_node()
        if (m == 0 || (it > 0 && __popcll(m) < kNodeMinLanes)) break;
        if (COUNT && lane0) {
            cnt.phase[1]++;
            cnt.phase[2] += (unsigned long long)__popcll(m);
        }
        const bool want = in_mask(m);
        ml.in_blas = in_mask(blas_m);
        if (want) tr.template node_step<true>(sc, st, cnt, &ml);
        if (COUNT && want) steps++;
        have_m = (have_m & ~m) | (m & __ballot(ml.k0 < Walk::kNoChild));
    }
    const unsigned long long lf = __ballot(tr.cur < 0), sm = __ballot(ml.top > base);
    const unsigned long long hv = act & have_m;
    unsigned long long wlm = hv & lf & blas_m, wim = hv & lf & ~blas_m;   // wants_leaf(), wants_instance()
    if (W4 && (tune.leaf_min_lanes > 1 || tune.inst_min_lanes > 1)) {
        const int nl = __popcll(wlm), ni = __popcll(wim);
        const bool nodes_left = ((hv & ~lf) | (act & ~have_m & sm)) != 0ull;
        const bool run_l = nl >= lmin || !(nodes_left || ni >= imin);
        const bool run_i = ni >= imin || !(nodes_left || (run_l && nl > 0));
        wlm = run_l ? wlm : 0ull;
        wim = run_i ? wim : 0ull;
    }
    if (COUNT) {
        const int nl = __popcll(wlm), ni = __popcll(wim);
        if (lane0 && nl) {
            cnt.phase[3]++;
            cnt.phase[4] += (unsigned long long)nl;
        }
        if (lane0 && ni) {
            cnt.phase[5]++;
            cnt.phase[6] += (unsigned long long)ni;
        }
    }
    const bool wl = in_mask(wlm), wi = in_mask(wim);
    if (wl) tr.leaf_step(sc, cnt);
    if (wi) tr.template instance_step<true>(sc, st, cnt, &ml);
    if (COUNT && (wl || wi)) steps++;
    // a leaf step leaves have = false and the stack as it was, an instance entry have = in_blas = true; everyone else is untouched
    have_m = (have_m & ~wlm) | wim;
    blas_m |= wim;
    wm.have = have_m;
    wm.in_blas = blas_m;
    return act & ~have_m & ~sm;   // active && !have && sp == 0 (an instance entry's push changes sp, but those lanes `have`)
}

// What a render writes once and reads once -- ray and hit queues, finished paths' colours, the framebuffers -- goes past the caches
// with the non-temporal hint (`nt` on the load / store), so that 200 MB of hand-offs per launch do not push the tree's records out
// of the 4 MB L2s (C3 -2.5 %, the 4 M-triangle scene -3 %: round 5).
typedef float jpt_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t jpt_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 stream_ld4(const float4* p)
{
    const jpt_v4f v = __builtin_nontemporal_load(reinterpret_cast<const jpt_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stream_st4(float4* p, const float4 v)
{
    jpt_v4f w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<jpt_v4f*>(p));
}
__device__ __forceinline__ uint4 stream_ldu4(const uint4* p)
{
    const jpt_v4u v = __builtin_nontemporal_load(reinterpret_cast<const jpt_v4u*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stream_stf(float* p, const float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ uint32_t stream_ldu(const uint32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void stream_stu(uint32_t* p, const uint32_t v) { __builtin_nontemporal_store(v, p); }

constexpr uint32_t kHasRadiance = 0x80000000u;   // queue entry, direction.w: rad[path] holds the path's radiance (else it is 0)
constexpr uint32_t kPathMask = 0x7fffffffu;

struct Wf2Buffers {
    float4* ray_o[2];   // queue entry: origin.xyz, w = seed.y bits of the path (bounces >= 1)
    float4* ray_d[2];   // direction.xyz, w = path id bits | kHasRadiance
    float4* hit_a;      // t, u, v, tri bits          (same index as the ray)
    uint32_t* hit_b;    // inst | front << 31
    float4* thr_q[2];   // queue entry: the path's throughput.xyz, w = seed.x bits (dense, beside the ray: read with it)
    float4* thr;        // per path: where a set-aside path parks that float4 until wf2_finish (otherwise untouched)
    float4* rad;        // per path: radiance.xyz -- touched only by vertices that ADD radiance (emitters) and by paths that
                        // carry some (kHasRadiance in the queue entry): most vertices neither read nor write it
                        // (indexed by path; HDR_F32 mode: also the finished paths' output; w = seed.y of a set-aside path)
    uint32_t* fin8;     // REF_LDR8 mode: by path, the finished path's radiance as the rgba8 main.glsl:434 stores (4 bytes, not 16)
    float* first_depth; // per slot of the LAST frame: distance of the first hit (or far)
    uint32_t* qcount;   // [max_bounces + 2][kSegments] queue sizes; row b = rays traced in bounce b (b >= 1)
    uint32_t* redo_count;  // [0]: paths set aside because the reference cannot reach their hit (wf2_finish) ...
    float4* redo_rec;      // ... two float4 each: the vertex's ray, origin.w = bounce bits, direction.w = path id bits
    uint32_t redo_cap;     // records redo_rec holds (a few paths in 10^7 are set aside: not one record per path).  A hit
                           // that finds the buffer full is shaded as found -- the native tree's closest hit, without the
                           // reference's crack -- and counted in redo_count[1] (jpt_stats.set_aside_dropped)
};

// n / d for a divisor fixed per launch: one multiply-high with floor(2^32 / d) and one correction step (the
// estimate is never too large and at most one too small for n < 2^31) instead of the ~35-instruction emulated divide.
struct FastDiv {
    uint32_t d, m;
};
inline FastDiv make_fastdiv(uint32_t d) { return FastDiv{d ? d : 1u, d > 1u ? (uint32_t)(0x100000000ull / d) : 0xffffffffu}; }
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f)
{
    uint32_t q = __umulhi(n, f.m);
    const uint32_t r = n - q * f.d;
    return r >= f.d ? q + 1u : q;
}

struct Wf2Dims {
    // The paths of a render are those of the WINDOW: the tile-aligned rectangle of the image outside which every pixel is
    // sky-culled (the whole image when the cull is off).  Tiles, slots, chunks and path ids count inside it.
    int32_t tile_x0, tile_y0;  // the window's first tile (local tile rows)
    int32_t tiles_x, tiles_y;  // the window's size in tiles
    int32_t full_tiles_x, full_tiles_y;  // the context's whole share of the image in tiles (wf2_accumulate walks it)
    uint32_t tiles_per_frame;
    uint32_t slots_per_frame;  // tiles_per_frame * 64
    uint32_t n_chunks;         // tiles_per_frame * n_frames
    uint32_t seg_cap;          // entries per segment
    uint32_t run_shift;        // a segment is dealt runs of 2^run_shift consecutive chunks (neighbouring tiles of one frame)
    FastDiv by_tiles_x, by_full_tiles_x;
    FastDiv by_frames;         // path -> (slot, frame), path_slot_frame; wf2_accumulate: item -> (pixel, frame)
    int32_t acc_groups = 1;    // (wf2_accumulate: the frame groups whose blocks of rad / fin8 it reads, group_frames)
};

__device__ __forceinline__ void slot_to_pixel(uint32_t slot, const Wf2Dims& dm, int& px, int& ly)
{
    const uint32_t tile = slot >> 6, lane = slot & 63u;
    const uint32_t ty = fdiv(tile, dm.by_tiles_x), tx = tile - ty * (uint32_t)dm.tiles_x;
    const uint32_t ix = lane & 7u, iy = lane >> 3;
    px = (int)((tx + (uint32_t)dm.tile_x0) * 8u + ix);
    ly = (int)((ty + (uint32_t)dm.tile_y0) * 8u + iy);
}

// Path ids count (pixel slot, frame) pairs with the FRAME running fastest: path = slot * n_frames + frame (frames of the
// launch's group).  The primary launch deals a wave 64 consecutive ids -- every frame's sample of 64 / n_frames neighbouring
// pixels of one tile row -- so whatever is indexed by path (rad, fin8, thr) is touched in runs, by the primary launch and by
// the queues' order after it, and wf2_accumulate reads a pixel's frames as one run.
__device__ __forceinline__ void path_slot_frame(uint32_t path, const Wf2Dims& dm, uint32_t n_frames, uint32_t& slot, uint32_t& f)
{
    slot = fdiv(path, dm.by_frames);
    f = path - slot * n_frames;
}

// a path is over: its radiance goes where wf2_accumulate reads it -- in REF_LDR8 mode already as the rgba8 value of
// main.glsl:434 (the accumulation sums exactly those quantised values, progressive_rendering.glsl:33), 4 bytes per path
__device__ __forceinline__ void store_final(const Wf2Buffers& wb, int accum_mode, uint32_t p, f3 r)
{
    if (accum_mode == 0) stream_stu(&wb.fin8[p], unorm8(r.x) | (unorm8(r.y) << 8) | (unorm8(r.z) << 16));
    else stream_st4(&wb.rad[p], make_float4(r.x, r.y, r.z, 0.0f));
}

// Is pixel (px, py) outside the screen rectangles of all the boxes the TLAS root offers (SkyCull, jpt_kernels.h)?  Its
// primary ray then fails every box test of the root: sky.  Such (pixel, frame) paths are not stored anywhere: the primary
// launch skips them and wf2_accumulate recomputes their sky colour from (x, y, frame).
__device__ __forceinline__ bool sky_culled(const SkyCull& cull, int px, int py)
{
    bool outside = cull.n >= 0;
    for (int k = 0; k < 4; k++)
        if (k < cull.n && px >= cull.x0[k] && px <= cull.x1[k] && py >= cull.y0[k] && py <= cull.y1[k]) outside = false;
    return outside;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask, int lane)
{
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// ---- a long walk, finished by a whole wave -----------------------------------------------------------------------------
//
// A launch cannot end before its longest ray does, and a lone ray advances one dependent fetch at a time (~0.8 us a step on an
// otherwise idle chip).  On the 1 M-triangle scene 40 of 16.6 M primary rays take 1 000 - 5 310 record steps (99.99 % take
// fewer than 256): the primary launch spent 4.4 of its 7.6 ms waiting for them (profiles/r04/r04g_tail_probe.txt,
// r04h_walk_hist.txt).  coop_walk walks ONE ray with all 64 lanes of a wave, again from the root: a lane walks one subtree with
// its private stack, gives the entry on top of that stack to the wave's pool (LDS) whenever lanes are idle, idle lanes take
// entries from the pool (an entry carries its level: TLAS, or the instance it belongs to), and after every round all lanes adopt
// the closest distance any of them has found, so every lane culls with it.  The closest hit does not depend on the order of the
// tests; two lanes that both keep a triangle at the final distance are an exact tie and flagged as one (kHitTied), like two such
// triangles met by one walk.  5 310 dependent steps become ~150 rounds: S-unique's primary launch 8.9 -> 4.2 ms (profiles/r04/
// r04l_coop_ab.txt).  Used as the TAIL phase of the tracing launches on scenes of >= 200 000 triangles: on the small scenes no ray
// is long and the launches' tails are the drain of ordinary rays.  (Round 4's other form -- the long rays listed and walked by a
// follow-up launch, wf2_long -- cost small renders 15 % in empty launches and was removed in round 6: LAB_NOTEBOOK.md.)
constexpr int kCoopPool = 64;      // pool entries per wave (two words each)

__device__ __forceinline__ float wave_min_f(float v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmin_(v, __shfl_xor(v, off));
    return v;
}

// (`pool`: 2 * kCoopPool words of LDS, word w at pool[(w >> 6) * pool_stride + (w & 63)] -- a flat array with pool_stride = 64,
// or two rows of the block's stack array, see the tail phase of the tracing kernels)
template <bool COUNT>
__device__ __forceinline__ TraceHit coop_walk(const WideSceneDev& sc, const typename Traversal<COUNT, true>::Stack st, int32_t* __restrict__ pool,
                                           f3 ro, f3 rd, DevCounters& cnt, const uint32_t pool_stride = 64u)
{
    using Walk = Traversal<COUNT, true>;
    const int lane = threadIdx.x & 63;
    auto pw = [&](uint32_t w) -> int32_t& { return pool[(w >> 6) * pool_stride + (w & 63u)]; };
    constexpr uint32_t kNone = 0xffffffffu;   // hit.tri of a lane that holds no triangle of its own at hit.t
    Walk tr;
    tr.begin(sc, ro, rd);
    tr.hit.tri = kNone;
    bool active = lane == 0 && tr.have;
    if (lane != 0) tr.have = false;
    uint32_t n_pool = 0;
    uint32_t my_steps = 0;   // (counting builds: record steps of this lane; their sum is the walk's length, jpt_stats.walk_steps_*)
    for (;;) {
        // idle lanes take pool entries (newest first)
        {
            const unsigned long long idle = __ballot(!active);
            const uint32_t n_idle = (uint32_t)__popcll(idle);
            const uint32_t take = n_pool < n_idle ? n_pool : n_idle;
            if (take) {
                const uint32_t r = lanes_below(idle, lane);
                if (!active && r < take) {
                    const int32_t ref = pw(2u * (n_pool - 1u - r));
                    const uint32_t ctx = (uint32_t)pw(2u * (n_pool - 1u - r) + 1u);
                    tr.sp = 0;
                    tr.cur = ref;
                    tr.have = true;
                    tr.in_blas = (ctx & 1u) != 0u;
                    tr.cur_inst = ctx >> 1;
                    if (tr.in_blas) {   // the instance's local ray (instance_step's arithmetic, main.glsl:319-320)
                        const WideInstance* ip = sc.instances + tr.cur_inst;
                        const float4 m0 = ld4(&ip->inv[0]), m1 = ld4(&ip->inv[4]), m2 = ld4(&ip->inv[8]);
                        tr.o = mk3(m0.x * ro.x + m0.w * ro.y + m1.z * ro.z + m2.y, m0.y * ro.x + m1.x * ro.y + m1.w * ro.z + m2.z,
                                   m0.z * ro.x + m1.y * ro.y + m2.x * ro.z + m2.w);
                        tr.d = mk3(m0.x * rd.x + m0.w * rd.y + m1.z * rd.z, m0.y * rd.x + m1.x * rd.y + m1.w * rd.z,
                                   m0.z * rd.x + m1.y * rd.y + m2.x * rd.z);
                    } else {
                        tr.o = ro;
                        tr.d = rd;
                    }
                    tr.set_level();
                    active = true;
                }
                n_pool -= take;
            }
        }
        if (!__any(active)) break;   // (and the pool is empty: an idle lane would have taken from it)
        if (COUNT && active && (tr.have || tr.sp > 0)) my_steps++;
        if (active && !tr.step(sc, st, cnt)) active = false;
        // every lane culls with the closest distance found anywhere; a lane whose own triangle is farther no longer holds one
        {
            const float t = wave_min_f(tr.hit.t);
            if (t < tr.hit.t) {
                tr.hit.t = t;
                tr.hit.tri = kNone;
                tr.hit.inst = 0u;
            }
        }
        // while lanes are idle, lanes with pending entries give the one on top of their stack to the pool (never the sentinel
        // that marks "leave the instance": what lies above it belongs to the instance the lane is in)
        {
            const uint32_t n_idle = (uint32_t)__popcll(__ballot(!active));
            const uint32_t want = n_idle > n_pool ? n_idle - n_pool : 0u;
            if (want) {
                int32_t top = kSentinel;
                const bool may = active && tr.sp > 0;
                if (may) {   // peek
                    const int row = tr.sp - 1;
                    top = row < st.lds_entries ? st.lds[row * st.stride] : (row < st.lds_entries + st.spill_entries ? st.spill[row - st.lds_entries] : kSentinel);
                }
                const bool give = may && top != kSentinel;
                const unsigned long long gm = __ballot(give);
                const uint32_t r = lanes_below(gm, lane);
                const uint32_t room = (uint32_t)kCoopPool - n_pool;
                const uint32_t lim = want < room ? want : room;
                if (give && r < lim) {
                    tr.sp--;
                    pw(2u * (n_pool + r)) = top;
                    pw(2u * (n_pool + r) + 1u) = (int32_t)((tr.in_blas ? 1u : 0u) | (tr.cur_inst << 1));
                }
                const uint32_t given = (uint32_t)__popcll(gm);
                n_pool += given < lim ? given : lim;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) my_steps += (uint32_t)__shfl_xor((int)my_steps, off);
        if (lane == 0) count_walk(cnt, my_steps);
    }
    // the closest hit: the lanes that hold a triangle at the final distance
    const float best = wave_min_f(tr.hit.t);
    const unsigned long long win = __ballot(tr.hit.tri != kNone && tr.hit.t == best);
    TraceHit out;
    out.t = 1e9f;
    out.u = out.v = 0.0f;
    out.tri = out.inst = 0u;
    out.front = false;
    if (win && best < 1e9f) {
        // Several lanes holding a triangle at the final distance: WHICH lanes walked which subtrees depends on the pool's timing, so
        // the winner must not be "the lowest lane" -- without the reference's trees to re-decide the tie (watertight scenes,
        // uploads that are not in pre-order) the flagged winner is shaded as it is, and the image would depend on the schedule
        // (ADVICE r04).  The winner is a function of the ray alone: the largest triangle index, then the largest instance.
        unsigned long long pick = win;
        if (__popcll(win) > 1) {
            const bool mine = ((win >> lane) & 1ull) != 0ull;
            uint32_t kt = mine ? tr.hit.tri : 0u;
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)kt, off);
                kt = o > kt ? o : kt;
            }
            const bool top = mine && tr.hit.tri == kt;
            uint32_t ki = top ? ((tr.hit.inst >> kInstBits) & kInstMask) : 0u;
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)ki, off);
                ki = o > ki ? o : ki;
            }
            pick = __ballot(top && ((tr.hit.inst >> kInstBits) & kInstMask) == ki);
        }
        const int w = __ffsll((long long)pick) - 1;
        out.t = best;
        out.u = __shfl(tr.hit.u, w);
        out.v = __shfl(tr.hit.v, w);
        out.tri = (uint32_t)__shfl((int)tr.hit.tri, w);
        out.front = __shfl((int)tr.hit.front, w) != 0;
        const uint32_t wi = (uint32_t)__shfl((int)tr.hit.inst, w);
        const uint32_t found_in = (wi >> kInstBits) & kInstMask;
        const bool tied = __popcll(win) > 1 || (wi & kHitTied) != 0u;
        out.inst = found_in | (found_in << kInstBits) | (tied ? kHitTied : 0u);
    }
    return out;
}

// The walk as the TAIL of a tracing launch: a wave whose block's queue has been dry for
// `tail_rounds` rounds and that is down to `tail_lanes` rays stops walking them lane by lane -- a lone ray advances one dependent
// step per microsecond, and a small render's launches each last as long as their longest walk (tools/step_latency.py: 64 x 64
// pixels, longest walk 42 steps, launch 48 us; 1920 x 1080 x 1: 102 steps, 110 us) -- and walks them one after the other with
// all its lanes, again from the root.  The call is OUT OF LINE so that the walk's registers are not the hot loop's (inlined
// there it cost the loop spills and every launch 10-20 %, round 4); its pool is the top two rows of the wave's own columns of
// the block's stack array, its private stacks the rows below.
template <bool COUNT>
__device__ __attribute__((noinline)) void coop_walk_call(const WideSceneDev* __restrict__ scp, int32_t* lds_col, int32_t* pool, float ox, float oy,
                                                         float oz, float dx, float dy, float dz, DevCounters* cntp, TraceHit* out)
{
    int32_t spill[kStackSpill + 2];   // (the two LDS rows the pool takes are made up for here)
    const typename Traversal<COUNT, true>::Stack st{lds_col, spill, kTraceBlock, kStackLds - 2, kStackSpill + 2};
    const WideSceneDev sc = *scp;
    DevCounters none = {};
    *out = coop_walk<COUNT>(sc, st, pool, mk3(ox, oy, oz), mk3(dx, dy, dz), COUNT ? *cntp : none, (uint32_t)kTraceBlock);
}

// ---- bounces >= 1: trace the segment's ray queue ----------------------------------------------------------

// `chain` consecutive segments are one block's queue (entries of segment seg0, then seg0 + 1, ...): the grid is
// kSegments / chain blocks.  A deeper queue per block keeps the lanes refilled for a larger share of the launch (at
// bounce 4 of C3 a segment holds 1.7 rays per lane); the slots this leaves free are used by the launches of the
// other renders in flight (render pipelining), so chain > 1 only pays when renders are queued.
#ifndef JPT_MAX_CHAIN
#define JPT_MAX_CHAIN 4
#endif
constexpr int kMaxChain = JPT_MAX_CHAIN;
// The walk of one block's ray queue -- `n` entries in the consecutive segments seg0, seg0 + 1, .. (end[k] = entries in the first k + 1
// of them) -- with the block's stack columns and queue cursor in LDS: the body of wf2_trace.
template <bool COUNT, bool W4, bool TAIL>
__device__ __forceinline__ void trace_queue(const WideSceneDev& sc, const Wf2Buffers& wb, const Wf2Dims& dm, const int bounce, const WfTune& tune,
                                            const uint32_t seg0, const uint32_t (&end)[kMaxChain], const uint32_t n, int32_t* __restrict__ stack,
                                            uint32_t* __restrict__ s_cursor, DevCounters& cnt)
{
    const int lane = threadIdx.x & 63;
    int32_t spill[kStackSpill];
    const typename Traversal<COUNT, W4>::Stack my_stack{&stack[threadIdx.x], spill, kTraceBlock, kStackLds};
    uint32_t dry_rounds = 0;   // (TAIL: rounds of this wave since the block's queue ran dry; wave-uniform)
    const float4* __restrict__ qo = wb.ray_o[bounce & 1];
    const float4* __restrict__ qd = wb.ray_d[bounce & 1];
    Traversal<COUNT, W4> tr;
    tr.cur = 0;
    // the walk's flags as lane masks and the stack position as an LDS address (walk_round_masked); tr.have / in_blas / sp are not used
    WalkMasks wm;
    typename Traversal<COUNT, W4>::Masked ml;
    ml.top = Traversal<COUNT, W4>::lds_base(my_stack);
    ml.k0 = 0u;
    ml.in_blas = false;
    // The wave's bookkeeping is wave-uniform and lives in scalars: `act`, the lanes that hold a ray -- the round takes the
    // finished ones out, the refill adds the ones it filled; idle lanes, the exit tests and the tail's lanes all derive from it --
    // and `unsaved`, the lanes whose finished walk has not written its hit yet.
    unsigned long long act = 0ull, unsaved = 0ull;
    bool exhausted = false;
    size_t my_loc = 0;
    uint32_t walk_steps = 0;   // (counting builds: record steps of this lane's ray)
    // A finished walk's hit stays in the lane's registers until the lane takes its next ray: the hits are written when the
    // wave refills (two dozen lanes at once) instead of in the round each walk happens to end in (some lane does in
    // nearly every round: a dozen instructions per round for one or two lanes' stores).
    auto save_hit = [&]() {
        stream_st4(&wb.hit_a[my_loc], make_float4(tr.hit.t, tr.hit.u, tr.hit.v, __uint_as_float(tr.hit.tri)));
        stream_stu(&wb.hit_b[my_loc], tr.hit.inst | (tr.hit.front ? 0x80000000u : 0u));
    };

    for (;;) {
        const unsigned long long idle = ~act;
        const int n_idle = __popcll(idle);
        if (!exhausted && n_idle >= tune.refill_idle) {
            if (in_mask(unsaved)) save_hit();
            unsaved = 0ull;
            uint32_t start = 0;
            if (lane == 0) start = atomicAdd(s_cursor, (uint32_t)n_idle);
            start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
            if (start + (uint32_t)n_idle >= n) exhausted = true;
            if (start < n) {
                const uint32_t idx = start + lanes_below(idle, lane);
                const unsigned long long fill = idle & __ballot(idx < n);
                if (in_mask(fill)) {
                    // which of the chained segments holds entry idx
                    uint32_t k = 0, first = 0;
                    for (int j = 0; j < kMaxChain - 1; j++)
                        if (idx >= end[j]) {
                            k = (uint32_t)j + 1u;
                            first = end[j];
                        }
                    const size_t loc = (size_t)(seg0 + k) * dm.seg_cap + (idx - first);
                    const float4 ro = stream_ld4(&qo[loc]), rd = stream_ld4(&qd[loc]);
                    tr.begin(sc, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z));
                    ml.top = Traversal<COUNT, W4>::lds_base(my_stack);   // begin()'s sp = 0
                    my_loc = loc;
                    walk_steps = 0;
                }
                act |= fill;
                wm.have = sc.n_instances != 0 ? (wm.have | fill) : (wm.have & ~fill);   // begin()'s have and in_blas
                wm.in_blas &= ~fill;
            }
        }
        if (act == 0ull) {
            if (exhausted) break;
            continue;
        }
        {
            const unsigned long long done = walk_round_masked<COUNT, W4>(tr, ml, wm, act, sc, my_stack, cnt, tune, walk_steps);
            act &= ~done;
            unsaved |= done;
            if (COUNT) {
                if (in_mask(done)) count_walk(cnt, walk_steps);
            }
            if constexpr (TAIL && W4) {
                if (exhausted && ++dry_rounds >= (uint32_t)tune.tail_rounds && __popcll(act) <= tune.tail_lanes) break;
            }
        }
    }
    if constexpr (TAIL && W4) {
        // tail phase (see wf2_primary)
        unsigned long long left = act;
        if (left) {
            if (in_mask(unsaved)) save_hit();
            unsaved = 0ull;
            const int wave_col = (int)(threadIdx.x & ~63u);
            while (left) {
                const int src = __ffsll((long long)left) - 1;
                left &= left - 1ull;
                TraceHit h;
                const WideSceneDev sc_tail = sc;   // (a copy of its own: `sc` itself must not have its address taken, or the hot loop reads it from scratch)
                coop_walk_call<COUNT>(&sc_tail, &stack[threadIdx.x], &stack[(kStackLds - 2) * kTraceBlock + wave_col], __shfl(tr.wo.x, src),
                                      __shfl(tr.wo.y, src), __shfl(tr.wo.z, src), __shfl(tr.wd.x, src), __shfl(tr.wd.y, src), __shfl(tr.wd.z, src),
                                      COUNT ? &cnt : nullptr, &h);
                if (lane == src) {
                    tr.hit = h;
                    save_hit();
                }
            }
        }
    }
    if (in_mask(unsaved)) save_hit();
}

template <bool COUNT, bool W4, bool TAIL = false>
__global__ __launch_bounds__(kBlock, JPT_WAVES_PER_SIMD) void wf2_trace(WideSceneDev sc, Wf2Buffers wb, Wf2Dims dm, int bounce, WfTune tune,
                                                    int chain, DevCounters* __restrict__ counters)
{
    __shared__ int32_t stack[kStackLds * kBlock];
    __shared__ uint32_t s_cursor;
    const uint32_t seg0 = blockIdx.x * (uint32_t)chain;
    // end[k] = entries in segments seg0 .. seg0 + k (wave-uniform, kept in scalars)
    uint32_t end[kMaxChain];
    uint32_t n = 0;
    for (int k = 0; k < kMaxChain; k++) {
        if (k < chain && seg0 + (uint32_t)k < kSegments) n += wb.qcount[(size_t)bounce * kSegments + seg0 + (uint32_t)k];
        end[k] = n;
    }
    if (n == 0) return;
    if (threadIdx.x == 0) s_cursor = 0;
    __syncthreads();
    DevCounters cnt = {};
    trace_queue<COUNT, W4, TAIL>(sc, wb, dm, bounce, tune, seg0, end, n, stack, &s_cursor, cnt);
    if (COUNT) flush_counters(cnt, counters);
}

// ---- the sky cells of culled pixels (wf2_accumulate; the argument is there) -------------------------------------------------
constexpr float kCellMargin = 0.01f;
// values * 255 + 0.5 of the sky along the ray through a raster position, per channel; false: the camera block does not behave
// there (the clip-space w changes sign against `w_ref`, or a NaN).  (raster_direction_approx: reciprocal estimates instead of six
// divisions and a square root -- a few ulp of d.y, i.e. 1e-5 of a cell against kCellMargin = 1e-2.)
__device__ __forceinline__ bool sky_cells_at(const RefCamera& cam, float two_over_w, float two_over_h, float fx, float fy, float w_ref, float& w_out,
                                             float v[3], f3& d)
{
    d = raster_direction_approx(cam, two_over_w, two_over_h, fx, fy, w_out);
    const f3 c = mk3(0.0f, 0.0f, 0.0f) + mk3(1.0f, 1.0f, 1.0f) * sample_sky(d);
    v[0] = clamp_(c.x, 0.0f, 1.0f) * 255.0f + 0.5f;
    v[1] = clamp_(c.y, 0.0f, 1.0f) * 255.0f + 0.5f;
    v[2] = clamp_(c.z, 0.0f, 1.0f) * 255.0f + 0.5f;
    return (w_out * w_ref > 0.0f) && (d.y == d.y);   // (callers that compare the signs themselves pass w_ref = 1)
}
// how far d.y can leave the range of the four corner values inside the quadrilateral, in cells; 1e30 when it is too wide to bound
__device__ __forceinline__ float sky_interior_excess(const f3 c[4])
{
    float chord2 = 0.0f, ay = 0.0f;
    for (int i = 0; i < 4; i++) {
        ay = fmax_(ay, __builtin_fabsf(c[i].y));
        for (int j = i + 1; j < 4; j++) {
            const f3 e = c[i] - c[j];
            chord2 = fmax_(chord2, e.x * e.x + e.y * e.y + e.z * e.z);
        }
    }
    if (!(chord2 < 0.2f)) return 1e30f;                        // (also a NaN)
    const float theta2 = 1.1f * chord2;                        // theta <= 0.5: theta^2 < 1.03 chord^2
    const float m = fmin_(1.0f, ay + __builtin_sqrtf(theta2));  // max |d.y| inside: a corner's, plus at most theta
    return 6.4f * 0.25f * theta2 * m;
}

// The TILE-level test of wf2_accumulate as a pass of its own, one LANE per 8 x 8 tile instead of one wave (round 5): do the four
// corner rays of the tile agree on one rgba8 sky cell per channel, with the margins of the argument in wf2_accumulate?  Then every
// culled pixel of the tile has that value for all its frames: tile_cell = 0x80000000 | r | g << 8 | b << 16; else 0 (the tile's
// culled pixels are decided one by one, or take the exact route).  Depends on the camera, the image size and the partition only:
// the host runs it when one of those changes (jpt_capi.cpp), not per render -- 32 400 lanes once per camera instead of 32 400 waves
// x ~300 instructions in every accumulation.
__global__ __launch_bounds__(kBlock) void wf2_sky_tiles(Wf2Dims dm, FrameParams fp, RefCamera cam, uint32_t* __restrict__ tile_cell)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint32_t)dm.full_tiles_x * (uint32_t)dm.full_tiles_y) return;
    const uint32_t fty = fdiv(t, dm.by_full_tiles_x), ftx = t - fty * (uint32_t)dm.full_tiles_x;
    const int tx0 = (int)ftx * 8, ty0 = local_to_global_row((int)fty * 8, fp);
    const float two_over_w = 2.0f / (float)fp.width, two_over_h = 2.0f / (float)fp.height;
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    f3 cd[4];
    float w0 = 1.0f;
    bool ok = true;
    for (int corner = 0; corner < 4; corner++) {
        float ww, v[3];
        (void)sky_cells_at(cam, two_over_w, two_over_h, (float)(tx0 + 8 * (corner & 1)), (float)(ty0 + 8 * (corner >> 1)), 1.0f, ww, v, cd[corner]);
        if (corner == 0) w0 = ww;
        ok = ok && (ww == ww) && (v[0] == v[0]) && (ww * w0 > 0.0f);   // no NaN, and the four w of one sign
        for (int k = 0; k < 3; k++) {
            lo[k] = fmin_(lo[k], v[k]);
            hi[k] = fmax_(hi[k], v[k]);
        }
    }
    const float excess = sky_interior_excess(cd);
    uint32_t cell = 0x80000000u;
    for (int k = 0; k < 3; k++) {
        const float l = lo[k] - excess, h = hi[k] + excess;
        const float c = __builtin_floorf(l);
        ok = ok && (l - c >= kCellMargin) && (h - c <= 1.0f - kCellMargin) && (h - l < 0.5f);
        cell |= ((uint32_t)c & 255u) << (8 * k);
    }
    tile_cell[t] = ok ? cell : 0u;
}

// ---- next-event estimation of the environment map (JPT_ENV_SAMPLING_MIS) ----------------------------------------------------

// The MIS pipeline's own buffers, carved behind the rest of the layout (wf2_layout) and passed to its kernels only
struct Wf2Nee {
    float4* sh_o;       // shadow queue entry ([segment][entry], as the ray queues): origin.xyz, w = path id bits | kNeeFinal
    float4* sh_d;       // the map direction
    float4* sh_c;       // the contribution if unoccluded
    uint32_t* scount;   // [max_bounces][kSegments] shadow rays queued by wf2_shade_mis of bounce b (zeroed at the render's start)
    float* pdf;         // per path: the BRDF density of its last sampled direction (the weight of a miss at the next vertex)
};
constexpr uint32_t kNeeFinal = 0x80000000u;   // the path ended at the vertex that cast the shadow ray: its final value is stored here

// a shadow ray has been traced: the unoccluded contribution joins rad[path]; a path that ended at the vertex is stored
__device__ __forceinline__ void nee_land(const Wf2Buffers& wb, int accum_mode, const float4 so, const float4 sc4, bool blocked)
{
    const uint32_t w = __float_as_uint(so.w), p = w & kPathMask;
    const float4 r4 = wb.rad[p];
    f3 r = mk3(r4.x, r4.y, r4.z);
    if (!blocked) r = r + mk3(sc4.x, sc4.y, sc4.z);
    if (w & kNeeFinal) store_final(wb, accum_mode, p, r);
    else if (!blocked) wb.rad[p] = make_float4(r.x, r.y, r.z, 0.0f);
}

// The shadow rays wf2_shade_mis queued at `bounce`: one lane per ray, the closest-hit walk of the native tree stopped at its first
// accepted triangle ("blocked": some triangle's Moller-Trumbore test accepts t <= 1e9, no reach or tie logic -- on the native tree
// the brute-force answer).  The whole stack is in LDS (one wave per block): no scratch.  Runs between wf2_shade_mis of `bounce` and
// that of bounce + 1, so the contributions join each path's radiance in vertex order.
constexpr int kOccBlock = 64;
template <bool COUNT, bool W4>
__global__ __launch_bounds__(kOccBlock) void wf2_occlude(WideSceneDev sc, Wf2Buffers wb, Wf2Dims dm, FrameParams fp, int bounce, Wf2Nee nee,
                                                         DevCounters* __restrict__ counters)
{
    constexpr int kDepth = kStackLds + kStackSpill;
    __shared__ int32_t stack[kDepth * kOccBlock];
    const uint32_t seg = blockIdx.y;
    const uint32_t i = blockIdx.x * kOccBlock + threadIdx.x;
    if (i >= nee.scount[(size_t)bounce * kSegments + seg]) return;
    const size_t at = (size_t)seg * dm.seg_cap + i;
    const float4 so = stream_ld4(&nee.sh_o[at]), sd = stream_ld4(&nee.sh_d[at]), sc4 = stream_ld4(&nee.sh_c[at]);
    const typename Traversal<COUNT, W4>::Stack st{&stack[threadIdx.x], nullptr, kOccBlock, kDepth, 0};
    DevCounters cnt = {};
    Traversal<COUNT, W4> tr;
    tr.begin(sc, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z));
    while (tr.hit.t >= 1e9f && tr.step(sc, st, cnt)) {
    }
    nee_land(wb, fp.accum_mode, so, sc4, tr.hit.t < 1e9f);
    if (COUNT) flush_counters(cnt, counters);
}

// The emitters' shadow rays (JPT_LIGHT_SAMPLING_MIS) that wf2_shade_lt queued at `bounce`: wf2_occlude's walk, started with
// hit.t = tmax (the entry's direction w), so boxes and triangles beyond it are pruned: "blocked" when some triangle's
// Moller-Trumbore test accepts t < tmax (the walk ends with hit.t < tmax).  Runs after that bounce's wf2_occlude (the map's shadow
// rays of the same vertices): two rays of one vertex never share a launch.
template <bool COUNT, bool W4>
__global__ __launch_bounds__(kOccBlock) void wf2_occlude_lt(WideSceneDev sc, Wf2Buffers wb, Wf2Dims dm, FrameParams fp, int bounce, Wf2Nee nee,
                                                            DevCounters* __restrict__ counters)
{
    constexpr int kDepth = kStackLds + kStackSpill;
    __shared__ int32_t stack[kDepth * kOccBlock];
    const uint32_t seg = blockIdx.y;
    const uint32_t i = blockIdx.x * kOccBlock + threadIdx.x;
    if (i >= nee.scount[(size_t)bounce * kSegments + seg]) return;
    const size_t at = (size_t)seg * dm.seg_cap + i;
    const float4 so = stream_ld4(&nee.sh_o[at]), sd = stream_ld4(&nee.sh_d[at]), sc4 = stream_ld4(&nee.sh_c[at]);
    const typename Traversal<COUNT, W4>::Stack st{&stack[threadIdx.x], nullptr, kOccBlock, kDepth, 0};
    DevCounters cnt = {};
    Traversal<COUNT, W4> tr;
    tr.begin(sc, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z));
    const float tmax = sd.w;
    tr.hit.t = tmax;
    while (tr.hit.t >= tmax && tr.step(sc, st, cnt)) {
    }
    nee_land(wb, fp.accum_mode, so, sc4, tr.hit.t < tmax);
    if (COUNT) flush_counters(cnt, counters);
}

// the kernels that see the paths' misses (jpt_wf2_paths.h): the default ones, the *_env ones, the *_mis ones, the *_lt ones, then the *_tx ones
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 2
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 3
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 4
#include "jpt_wf2_paths.h"
#undef JPT_ENV
// ... and the lens forms of the two bounce-0 kernels (jpt_set_lens): wf2_primary_lens, wf2_primary_env_lens
#define JPT_LENS 1
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#undef JPT_LENS
// ... and their camera-model forms (jpt_set_camera_model): wf2_primary_cam, wf2_primary_env_cam
#define JPT_CAMERA_MODEL 1
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#undef JPT_CAMERA_MODEL
// ... and their bake forms (jpt_set_bake_texels): wf2_primary_bake, wf2_primary_env_bake
#define JPT_BAKE 1
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#undef JPT_BAKE
// ... and their probe forms (jpt_set_probes): wf2_primary_probe, wf2_primary_env_probe
#define JPT_PROBE 1
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#undef JPT_PROBE
// ... and their cube forms (jpt_set_reflection_probes): wf2_primary_cube, wf2_primary_env_cube
#define JPT_CUBE 1
#define JPT_ENV 0
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#define JPT_ENV 1
#include "jpt_wf2_paths.h"
#undef JPT_ENV
#undef JPT_CUBE

// the window of a render (local tiles): x0, y0, nx, ny
struct TileWindow {
    int x0, y0, nx, ny;
};
TileWindow full_window(int width, int local_rows) { return TileWindow{0, 0, (width + 7) / 8, (local_rows + 7) / 8}; }

// The tile-aligned bounding rectangle of the cull's screen rectangles, in this context's local tile rows (8-row strips
// s with s % world == rank: local tile row t is image tile row t * world + rank).  Outside it every pixel is
// sky-culled, so no path starts there.  Nothing visible at all: one tile (its pixels are culled one by one).
TileWindow cull_window(const SkyCull& cull, const FrameParams& fp)
{
    const TileWindow full = full_window(fp.width, fp.local_rows);
    if (cull.n < 0) return full;
    const TileWindow none{0, 0, 1, 1};
    int gx0 = INT32_MAX, gy0 = INT32_MAX, gx1 = INT32_MIN, gy1 = INT32_MIN;
    for (int k = 0; k < 4 && k < cull.n; k++) {
        if (cull.x0[k] > cull.x1[k] || cull.y0[k] > cull.y1[k]) continue;
        gx0 = std::min(gx0, cull.x0[k]);
        gy0 = std::min(gy0, cull.y0[k]);
        gx1 = std::max(gx1, cull.x1[k]);
        gy1 = std::max(gy1, cull.y1[k]);
    }
    gx0 = std::max(gx0, 0);
    gy0 = std::max(gy0, 0);
    gx1 = std::min(gx1, fp.width - 1);
    gy1 = std::min(gy1, fp.height - 1);
    if (gx0 > gx1 || gy0 > gy1) return none;
    const int world = fp.world > 0 ? fp.world : 1;
    const int ty0 = gy0 / 8 - fp.rank, ty1 = gy1 / 8 - fp.rank;   // image tile rows, shifted so that this rank's are the multiples of world
    if (ty1 < 0) return none;
    const int lt0 = ty0 <= 0 ? 0 : (ty0 + world - 1) / world, lt1 = std::min(ty1 / world, full.ny - 1);
    if (lt0 > lt1) return none;
    return TileWindow{gx0 / 8, lt0, gx1 / 8 - gx0 / 8 + 1, lt1 - lt0 + 1};
}

Wf2Dims make_dims(int width, int local_rows, int n_frames, const TileWindow& win)
{
    Wf2Dims dm;
    dm.tile_x0 = win.x0;
    dm.tile_y0 = win.y0;
    dm.tiles_x = win.nx;
    dm.tiles_y = win.ny;
    dm.full_tiles_x = (width + 7) / 8;
    dm.full_tiles_y = (local_rows + 7) / 8;
    dm.by_full_tiles_x = make_fastdiv((uint32_t)dm.full_tiles_x);
    dm.tiles_per_frame = (uint32_t)dm.tiles_x * (uint32_t)dm.tiles_y;
    dm.slots_per_frame = dm.tiles_per_frame * 64u;
    dm.n_chunks = dm.tiles_per_frame * (uint32_t)n_frames;
    // Chunks are dealt to the segments in runs of 2^run_shift consecutive chunks -- consecutive parts of one tile, whose rays stay
    // alike for longer -- but runs also unbalance the segments: single chunks up to a few hundred per segment, runs of two / four
    // only for the largest renders (3840 x 2160 x 16: 1 157 chunks per segment).  Swept in rounds 1-4: LAB_NOTEBOOK.md.
    const uint32_t per_segment = dm.n_chunks / kSegments;
    const uint32_t run_shift = per_segment >= 512u ? 2u : (per_segment >= 256u ? 1u : 0u);
    dm.run_shift = run_shift;
    const uint32_t n_runs = (dm.n_chunks + (1u << run_shift) - 1u) >> run_shift;
    dm.seg_cap = (((n_runs + kSegments - 1u) / kSegments) << run_shift) * 64u;
    dm.by_tiles_x = make_fastdiv((uint32_t)dm.tiles_x);
    dm.by_frames = make_fastdiv((uint32_t)(n_frames > 0 ? n_frames : 1));
    return dm;
}

}  // namespace

size_t wf2_sky_tile_count(int width, int local_rows) { return (size_t)((width + 7) / 8) * (size_t)((local_rows + 7) / 8); }
void launch_sky_tiles(hipStream_t stream, const FrameParams& fp, const RefCamera& cam, uint32_t* tile_cell)
{
    const Wf2Dims dm = make_dims(fp.width, fp.local_rows, 1, full_window(fp.width, fp.local_rows));
    const uint32_t n_tiles = (uint32_t)dm.full_tiles_x * (uint32_t)dm.full_tiles_y;
    if (n_tiles) hipLaunchKernelGGL(wf2_sky_tiles, dim3((n_tiles + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, dm, fp, cam, tile_cell);
}
uint32_t wf2_segments() { return kSegments; }
uint32_t trace_stack_capacity() { return (uint32_t)(kStackLds + kStackSpill); }

// Frame groups: the frames of a render split into groups, each running the pipeline on its own stream with its own queues
// (the rule and its measurements: plan_launch, jpt_capi.cpp).  Paths never cross groups and the per-pixel accumulation still
// reads the frames in order: results are unchanged.
static void group_frames(int n_frames, int groups, int g, int& first, int& count)
{
    const int base = n_frames / groups, extra = n_frames % groups;
    first = g * base + (g < extra ? g : extra);
    count = base + (g < extra ? 1 : 0);
}

// Set-aside records per group: a path is set aside at most once, and few are (float cracks of the reference's boxes: a
// handful per render; exact distance ties: rare outside scenes built of coincident geometry): 1/64 of the paths, at least
// 65 536 (2 MB) and never more than the paths, instead of one 32-byte record per path (0.5 GB per pipeline slot at C3).
// Overflow is counted, not silent: jpt_stats.set_aside_dropped.
static uint32_t redo_capacity(size_t paths)
{
    if (tuning().set_aside_cap >= 0) return (uint32_t)std::min<size_t>((size_t)tuning().set_aside_cap, paths);   // (tests)
    const size_t c = std::min(paths, std::max<size_t>(paths / 64u, 65536u));
    return (uint32_t)(c > 0x7fffffffu ? 0x7fffffffu : c);
}

// The workspace of one render, carved from `base` in this order (group 0's queue sizes first: the host reads them).  The one
// layout there is: launch_wf2_render carves it from the real base, wf2_workspace_bytes from a null one for its size (the
// pointers are then offsets, never dereferenced).  wf2_primary owns the zeroing of the queue sizes of bounces >= 1 and of
// the set-aside counts: thread t of block s clears segment s's word of row t (1 <= t <= max_bounces + 1), and threads 192..
// of block 0 the 64 words behind the rows.
static_assert(kBlock >= 192 + 64, "wf2_primary clears the 64 set-aside words with threads 192.. of block 0");
static_assert(kMaxBounces + 1 < 192, "wf2_primary clears the queue-size rows with threads below 192");
struct Wf2Layout {
    Wf2Buffers gb[kMaxGroups];
    Wf2Dims gdm[kMaxGroups];
    FrameParams gfp[kMaxGroups];
    float4* rad;          // all groups' blocks, [slot][frame of the group] each
    uint32_t* fin8;
    float* first_depth;
    Wf2Nee gnee[kMaxGroups];   // (MIS renders only: carved behind everything else, so the other buffers stay where they are)
    Wf2Nee glnee[kMaxGroups];  // (light-sampling renders only: behind those; pdf shared with gnee when both are carved)
    size_t bytes = 0;     // the end of the last buffer
};
static Wf2Layout wf2_layout(void* base, const FrameParams& fp, int groups, const TileWindow& window, const Lighting& lg)
{
    Wf2Layout L;
    auto carve = [&](size_t bytes) {
        void* p = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(base) + L.bytes);
        L.bytes += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const int nq = fp.max_bounces + 2;
    const Wf2Dims dm_all = make_dims(fp.width, fp.local_rows, fp.n_frames, window);
    for (int g = 0; g < groups; g++) {
        L.gb[g].qcount = (uint32_t*)carve(((size_t)nq * kSegments + 64) * sizeof(uint32_t));   // queue sizes + the set-aside counts
        L.gb[g].redo_count = L.gb[g].qcount + (size_t)nq * kSegments;
    }
    L.rad = (float4*)carve((size_t)dm_all.slots_per_frame * (size_t)fp.n_frames * sizeof(float4));
    L.fin8 = (uint32_t*)carve((size_t)dm_all.slots_per_frame * (size_t)fp.n_frames * sizeof(uint32_t));
    L.first_depth = (float*)carve((size_t)dm_all.slots_per_frame * sizeof(float));
    for (int g = 0; g < groups; g++) {
        int f0, nf;
        group_frames(fp.n_frames, groups, g, f0, nf);
        L.gdm[g] = make_dims(fp.width, fp.local_rows, nf, window);
        const size_t q = (size_t)L.gdm[g].seg_cap * kSegments;
        const size_t paths = (size_t)L.gdm[g].slots_per_frame * (size_t)nf;
        Wf2Buffers& wb = L.gb[g];
        wb.ray_o[0] = (float4*)carve(q * sizeof(float4));
        wb.ray_o[1] = (float4*)carve(q * sizeof(float4));
        wb.ray_d[0] = (float4*)carve(q * sizeof(float4));
        wb.ray_d[1] = (float4*)carve(q * sizeof(float4));
        wb.thr_q[0] = (float4*)carve(q * sizeof(float4));
        wb.thr_q[1] = (float4*)carve(q * sizeof(float4));
        wb.hit_a = (float4*)carve(q * sizeof(float4));
        wb.hit_b = (uint32_t*)carve(q * sizeof(uint32_t));
        wb.redo_cap = redo_capacity(paths);
        wb.redo_rec = (float4*)carve((size_t)wb.redo_cap * 2 * sizeof(float4));
        wb.thr = (float4*)carve(paths * sizeof(float4));
        wb.rad = L.rad + (size_t)f0 * dm_all.slots_per_frame;  // this group's block behind the earlier groups'
        wb.fin8 = L.fin8 + (size_t)f0 * dm_all.slots_per_frame;
        wb.first_depth = L.first_depth;
        L.gfp[g] = fp;
        L.gfp[g].frame_index = fp.frame_index + (uint32_t)f0;
        L.gfp[g].n_frames = nf;
        L.gfp[g].depth_frame = (fp.depth_frame >= 0 && f0 + nf == fp.n_frames) ? nf - 1 : -1;  // the render's last frame writes the depth image (when there is one: jpt_set_outputs)
    }
    // the shadow queues of group g; their per-path densities are `shared`'s, or carved behind them
    auto carve_nee = [&](int g, const Wf2Nee* shared) {
        const size_t q = (size_t)L.gdm[g].seg_cap * kSegments;
        const size_t paths = (size_t)L.gdm[g].slots_per_frame * (size_t)L.gfp[g].n_frames;
        Wf2Nee ne;
        ne.sh_o = (float4*)carve(q * sizeof(float4));
        ne.sh_d = (float4*)carve(q * sizeof(float4));
        ne.sh_c = (float4*)carve(q * sizeof(float4));
        ne.scount = (uint32_t*)carve((size_t)(fp.max_bounces > 0 ? fp.max_bounces : 1) * kSegments * sizeof(uint32_t));
        ne.pdf = shared ? shared->pdf : (float*)carve(paths * sizeof(float));
        return ne;
    };
    const bool mis = lg.map_queues();
    for (int g = 0; g < groups && mis; g++) L.gnee[g] = carve_nee(g, nullptr);
    for (int g = 0; g < groups && lg.emitter_queues(); g++) {
        L.glnee[g] = carve_nee(g, mis ? &L.gnee[g] : nullptr);
        if (!mis) L.gnee[g] = Wf2Nee{nullptr, nullptr, nullptr, nullptr, L.glnee[g].pdf};
    }
    // (a *_tx render without emitter queues: its kernels queue no emitter shadow ray, but keep the per-path densities there)
    for (int g = 0; g < groups && lg.transmissive && !lg.emitter_queues(); g++) {
        float* pdf = mis ? L.gnee[g].pdf : (float*)carve((size_t)L.gdm[g].slots_per_frame * (size_t)L.gfp[g].n_frames * sizeof(float));
        L.glnee[g] = Wf2Nee{nullptr, nullptr, nullptr, nullptr, pdf};
        if (!mis) L.gnee[g] = L.glnee[g];
    }
    return L;
}

size_t wf2_workspace_bytes(int width, int local_rows, int n_frames, int max_bounces, const Lighting& lg)
{
    // every layout a render of this size may use: the largest of 1..kMaxGroups groups over the whole image
    FrameParams fp{};
    fp.width = width;
    fp.local_rows = local_rows;
    fp.n_frames = n_frames;
    fp.max_bounces = max_bounces;
    size_t worst = 0;
    for (int groups = 1; groups <= kMaxGroups && groups <= (n_frames < 1 ? 1 : n_frames); groups++)
        worst = std::max(worst, wf2_layout(nullptr, fp, groups, full_window(width, local_rows), lg).bytes);
    return worst;
}

namespace {
__global__ void add_queue_counts(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
}  // namespace

void launch_wf2_render(hipStream_t stream, const DeviceScene& ds, const FrameParams& fp, const RefCamera& cam, void* workspace,
                       float4* accum, uint32_t* ldr, float* depth, DevCounters* counters, hipEvent_t* trace_events,
                       const Wf2Render& r, int groups, int chain, const Wf2Streams& streams)
{
    const TileWindow window = cull_window(r.cull, fp);
    const Wf2Dims dm_all = make_dims(fp.width, fp.local_rows, fp.n_frames, window);
    if (dm_all.n_chunks == 0) return;
    const Lighting& lg = r.lighting;   // which of the kernel families of jpt_wf2_paths.h the launches take, and what they pass
    const Wf2Layout L = wf2_layout(workspace, fp, groups, window, lg);
    const int nq = fp.max_bounces + 2;

    const bool w4 = ds.use4;
    WideSceneDev sc;
    sc.blas_nodes = ds.blas_nodes;
    sc.tlas_nodes = ds.tlas_nodes;
    sc.nodesq = ds.nodesq;
    sc.tris = ds.wide_tris;
    sc.instances = w4 ? ds.wide_instances4 : ds.wide_instances;
    sc.tlas_root = w4 ? ds.tlas_root4 : ds.tlas_root;
    sc.n_instances = ds.n_instances;
    sc.reach_tri = ds.reach_tri;
    sc.reach_inst = ds.reach_inst;
    SceneShading sh = ds.shading();
    const dim3 block(kBlock);
    const WfTune tune{Tuning::refill_idle, Tuning::refill_idle, Tuning::node_min_lanes, Tuning::leaf_min_lanes, Tuning::inst_min_lanes, Tuning::phase_frac16, tuning().tail_rounds, tuning().tail_lanes};

    chain = chain < 1 ? 1 : (chain > kMaxChain ? kMaxChain : chain);
    const dim3 tgrid((kSegments + (uint32_t)chain - 1u) / (uint32_t)chain);
    const dim3 pgrid(kSegments);
    const int count = counters != nullptr;
    // The waves of a tracing launch finish their last, very long walks themselves, all lanes on one ray (the TAIL instantiations,
    // coop_walk_call): scenes large enough to have such walks (>= 200 000 triangles); JPT_TAIL=0 never, 1 on every scene.
    // walk: 0 two-child records, 1 four-child records, 2 four-child records with TAIL
    const int walk = !w4 ? 0 : ((tuning().tail < 0 ? ds.n_tris >= 200000u : tuning().tail != 0) ? 2 : 1);
    // the shading instantiations: the paths' last vertices without the BRDF code, scenes without a texture array without the
    // sampler code -- texmode 0 no texture array, 1 nearest filter, 2 linear filter (jpt.h: bit 1 of the sampler mode)
    const bool tex = sh.tex != nullptr && sh.n_layers > 0 && sh.tex_res > 0;
    const int texmode = !tex ? 0 : ((sh.sampler_mode & 2) ? 2 : 1);
    // wf2_finish decides exact distance ties on the reference's own trees (EXACT) where the scene keeps them, four-child walks only
    const TieShadowDev& sx = ds.x;
    const int finish_walk = !w4 ? 0 : (sx.ok ? 2 : 1);
    // the pipeline of one group on one stream
    auto run_group = [&](hipStream_t st, const Wf2Buffers& wb, const Wf2Dims& dm, const FrameParams& gp, const Wf2Nee& nee, const Wf2Nee& lnee,
                         hipEvent_t* ev) {
        // (the queue sizes of bounces >= 1 and the set-aside counts start from zero: wf2_primary clears them)
        // Blocks go to the 8 XCDs round-robin by linear index (y * grid.x + x), and the chunks of a segment are far from
        // alike (the first ones are full, the last ones empty): with grid.x a multiple of 8 every XCD would always get
        // the same chunk position.  An odd grid.x deals every position to every XCD (capping C3's grid.x from 37 to 8
        // cost 9 %).
        const dim3 sgrid(((dm.seg_cap + kBlock - 1) / kBlock) | 1u, kSegments), ogrid(((dm.seg_cap + kOccBlock - 1) / kOccBlock) | 1u, kSegments);
        if (lg.map_queues() && gp.max_bounces > 0) (void)hipMemsetAsync(nee.scount, 0, (size_t)gp.max_bounces * kSegments * sizeof(uint32_t), st);
        if (lg.emitter_queues() && gp.max_bounces > 0) (void)hipMemsetAsync(lnee.scount, 0, (size_t)gp.max_bounces * kSegments * sizeof(uint32_t), st);
        if (ev) (void)hipEventRecord(ev[0], st);
        with_consts<2, 3>([&](auto C, auto W) {
            const bool env = lg.env_mode != 0;   // (the primary launch is its miss model's: a primary miss has weight 1)
            switch (r.primary.kind) {   // (r.cull is off for every kind but the pinhole)
            case PrimaryRays::kLens:
                if (env) hipLaunchKernelGGL((wf2_primary_env_lens<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.lens, counters);
                else hipLaunchKernelGGL((wf2_primary_lens<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.lens, counters);
                break;
            case PrimaryRays::kCamModel:
                if (env) hipLaunchKernelGGL((wf2_primary_env_cam<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.cam_model, counters);
                else hipLaunchKernelGGL((wf2_primary_cam<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.cam_model, counters);
                break;
            case PrimaryRays::kBake:
                if (env) hipLaunchKernelGGL((wf2_primary_env_bake<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.bake, counters);
                else hipLaunchKernelGGL((wf2_primary_bake<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.bake, counters);
                break;
            case PrimaryRays::kProbe:
                if (env) hipLaunchKernelGGL((wf2_primary_env_probe<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.probe, counters);
                else hipLaunchKernelGGL((wf2_primary_probe<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.probe, counters);
                break;
            case PrimaryRays::kCube:
                if (env) hipLaunchKernelGGL((wf2_primary_env_cube<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.cube, counters);
                else hipLaunchKernelGGL((wf2_primary_cube<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.primary.cube, counters);
                break;
            case PrimaryRays::kPinhole:
                if (env) hipLaunchKernelGGL((wf2_primary_env<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.cull, counters);
                else hipLaunchKernelGGL((wf2_primary<C, W != 0, W == 2>), pgrid, block, 0, st, sc, wb, dm, gp, cam, tune, r.cull, counters);
                break;
            }
        }, count, walk);
        if (ev) (void)hipEventRecord(ev[1], st);
        for (int b = 0; b <= gp.max_bounces; b++) {
            with_consts<2, 2, 3>([&](auto C, auto LAST, auto TEX) {
                if (lg.transmissive) {
                    hipLaunchKernelGGL((wf2_shade_tx<C, LAST, TEX>), sgrid, block, 0, st, sh, wb, dm, gp, cam.far_, b, counters, lg.env, lg.samp, lg.lights, nee,
                                       lnee, lg.env_mode);
                    return;
                }
                switch (lg.kind) {
                case Lighting::kEmitters:
                    hipLaunchKernelGGL((wf2_shade_lt<C, LAST, TEX>), sgrid, block, 0, st, sh, wb, dm, gp, cam.far_, b, counters, lg.env, lg.samp, lg.lights, nee,
                                       lnee, lg.env_mode);
                    break;
                case Lighting::kMapMis:
                    hipLaunchKernelGGL((wf2_shade_mis<C, LAST, TEX>), sgrid, block, 0, st, sh, wb, dm, gp, cam.far_, b, counters, lg.env, lg.samp, nee);
                    break;
                case Lighting::kMap:
                    hipLaunchKernelGGL((wf2_shade_env<C, LAST, TEX>), sgrid, block, 0, st, sh, wb, dm, gp, cam.far_, b, counters, lg.env);
                    break;
                case Lighting::kSky:
                    hipLaunchKernelGGL((wf2_shade<C, LAST, TEX>), sgrid, block, 0, st, sh, wb, dm, gp, cam.far_, b, counters);
                    break;
                }
            }, count, b == gp.max_bounces, texmode);
            if (b == gp.max_bounces) break;
            if (lg.map_queues()) {
                with_consts<2, 3>([&](auto C, auto W) {
                    hipLaunchKernelGGL((wf2_occlude<C, W != 0>), ogrid, dim3(kOccBlock), 0, st, sc, wb, dm, gp, b, nee, counters);
                }, count, walk);
            }
            if (lg.emitter_queues()) {   // (after the map's: the emitters' shadow ray of a vertex lands second)
                with_consts<2, 3>([&](auto C, auto W) {
                    hipLaunchKernelGGL((wf2_occlude_lt<C, W != 0>), ogrid, dim3(kOccBlock), 0, st, sc, wb, dm, gp, b, lnee, counters);
                }, count, walk);
            }
            if (ev) (void)hipEventRecord(ev[2 * (b + 1)], st);
            with_consts<2, 3>([&](auto C, auto W) {
                hipLaunchKernelGGL((wf2_trace<C, W != 0, W == 2>), tgrid, block, 0, st, sc, wb, dm, b + 1, tune, chain, counters);
            }, count, walk);
            if (ev) (void)hipEventRecord(ev[2 * (b + 1) + 1], st);
        }
        if (sh.reach_tri) {  // the paths set aside because their hit is undecidable on the native tree: finished exactly
            const dim3 rgrid(256), rblock(64);   // (blocks past the set-aside count exit at once; more records than threads: grid-stride)
            with_consts<2, 3>([&](auto C, auto W) {
                if (lg.transmissive) {
                    hipLaunchKernelGGL((wf2_finish_tx<C, W != 0, W == 2>), rgrid, rblock, 0, st, sc, sx, sh, wb, dm, gp, cam.far_, counters, lg.env, lg.samp,
                                       lg.lights, nee, lnee, lg.env_mode);
                    return;
                }
                switch (lg.kind) {
                case Lighting::kEmitters:
                    hipLaunchKernelGGL((wf2_finish_lt<C, W != 0, W == 2>), rgrid, rblock, 0, st, sc, sx, sh, wb, dm, gp, cam.far_, counters, lg.env, lg.samp,
                                       lg.lights, nee, lnee, lg.env_mode);
                    break;
                case Lighting::kMapMis:
                    hipLaunchKernelGGL((wf2_finish_mis<C, W != 0, W == 2>), rgrid, rblock, 0, st, sc, sx, sh, wb, dm, gp, cam.far_, counters, lg.env, lg.samp, nee);
                    break;
                case Lighting::kMap:
                    hipLaunchKernelGGL((wf2_finish_env<C, W != 0, W == 2>), rgrid, rblock, 0, st, sc, sx, sh, wb, dm, gp, cam.far_, counters, lg.env);
                    break;
                case Lighting::kSky:
                    hipLaunchKernelGGL((wf2_finish<C, W != 0, W == 2>), rgrid, rblock, 0, st, sc, sx, sh, wb, dm, gp, cam.far_, counters);
                    break;
                }
            }, count, finish_walk);
        }
    };

    if (groups == 1) {
        run_group(stream, L.gb[0], L.gdm[0], L.gfp[0], L.gnee[0], L.glnee[0], trace_events);
    } else {
        // fork: the helper streams start after everything already queued on the context's stream
        (void)hipEventRecord(streams.fork, stream);
        for (int g = 1; g < groups; g++) (void)hipStreamWaitEvent(streams.aux_stream[g - 1], streams.fork, 0);
        // issue the groups' launches interleaved, so none of the streams runs ahead of the others on the host side
        // (run_group enqueues a whole pipeline; the hardware queues of the streams drain concurrently)
        for (int g = 0; g < groups; g++) run_group(g == 0 ? stream : streams.aux_stream[g - 1], L.gb[g], L.gdm[g], L.gfp[g], L.gnee[g], L.glnee[g], nullptr);
        // join, then fold the other groups' queue sizes into group 0's (the host reads those for the ray count)
        for (int g = 1; g < groups; g++) {
            (void)hipEventRecord(streams.join[g - 1], streams.aux_stream[g - 1]);
            (void)hipStreamWaitEvent(stream, streams.join[g - 1], 0);
        }
        const uint32_t nqc = (uint32_t)nq * kSegments + 2u;   // (and the two set-aside counts behind the queue sizes)
        for (int g = 1; g < groups; g++)
            hipLaunchKernelGGL(add_queue_counts, dim3((nqc + 255) / 256), dim3(256), 0, stream, L.gb[0].qcount, L.gb[g].qcount, nqc);
    }
    Wf2Buffers wb_all = L.gb[0];
    Wf2Dims dm_acc = dm_all;
    dm_acc.acc_groups = groups;
    wb_all.rad = L.rad;
    wb_all.fin8 = L.fin8;
    wb_all.first_depth = L.first_depth;
    // the accumulation touches the framebuffers: it waits for whatever ordered the context's renders before this one (before_acc)
    if (r.before_acc) (void)hipStreamWaitEvent(stream, r.before_acc, 0);
    // per-pixel variance (jpt_set_variance): the second moment of the per-frame values the accumulation is about to add, against the
    // sum as it stands BEFORE this render -- so in front of wf2_accumulate, on its stream (such a render has no sky cull: its window
    // is the whole share, and a slot is a pixel's place in the share)
    if (r.variance != nullptr) {
        VarianceArgs va;
        va.rad = L.rad;
        va.fin8 = L.fin8;
        va.accum = accum;
        va.plane = r.variance;
        va.full_tiles_x = dm_all.full_tiles_x;
        va.full_tiles_y = dm_all.full_tiles_y;
        va.slots_per_frame = dm_all.slots_per_frame;
        va.groups = groups;
        launch_variance_moments(stream, va, fp);
    }
    const uint32_t ablocks = ((uint32_t)dm_all.full_tiles_x * (uint32_t)dm_all.full_tiles_y * 64u + kBlock - 1) / kBlock;
    if (lg.env_mode != 0)   // (the accumulation is its miss model's too; with a map: no sky cells)
        hipLaunchKernelGGL(wf2_accumulate_env, dim3(ablocks), block, 0, stream, wb_all, dm_acc, fp, cam, r.cull, accum, ldr, depth, nullptr, lg.env);
    else
        hipLaunchKernelGGL(wf2_accumulate, dim3(ablocks), block, 0, stream, wb_all, dm_acc, fp, cam, r.cull, accum, ldr, depth, r.sky_tiles);
    // directional lightmaps (jpt_set_bake_directional): the moments of the same per-frame values, while the workspace still holds them
    // (a bake render has no sky cull: its window is the whole share, and a slot is a texel's place in the share)
    if (r.bake_dir != nullptr && r.primary.kind == PrimaryRays::kBake) {
        BakeDirArgs da;
        da.rad = L.rad;
        da.fin8 = L.fin8;
        da.normal = r.primary.bake.normal;
        da.planes = r.bake_dir;
        da.full_tiles_x = dm_all.full_tiles_x;
        da.full_tiles_y = dm_all.full_tiles_y;
        da.slots_per_frame = dm_all.slots_per_frame;
        da.groups = groups;
        launch_bake_moments(stream, da, fp);
    }
}

uint64_t wf2_pixels_outside_window(const SkyCull& cull, const FrameParams& fp)
{
    const TileWindow w = cull_window(cull, fp);
    const int64_t x0 = (int64_t)w.x0 * 8, x1 = std::min<int64_t>((int64_t)(w.x0 + w.nx) * 8, fp.width);
    const int64_t y0 = (int64_t)w.y0 * 8, y1 = std::min<int64_t>((int64_t)(w.y0 + w.ny) * 8, fp.local_rows);
    const int64_t inside = std::max<int64_t>(x1 - x0, 0) * std::max<int64_t>(y1 - y0, 0);
    return (uint64_t)((int64_t)fp.width * (int64_t)fp.local_rows - inside);
}

}  // namespace jpt
