// jpt_wf2_paths.h -- the kernels of jpt_kernels_wf2.hip that see the misses of the paths: wf2_primary, wf2_shade (and shade_entry,
// which wf2_finish shares), wf2_finish and wf2_accumulate.  Included five times by jpt_kernels_wf2.hip, inside its anonymous namespace
// (and twice more with JPT_LENS defined, twice with JPT_CAMERA_MODEL, twice with JPT_BAKE, twice with JPT_PROBE and twice with JPT_CUBE, for the lens,
// camera-model, bake, probe and cube forms of wf2_primary alone: see there):
//   JPT_ENV 0   the default kernels, whose misses see main.glsl's gradient (sample_sky): the same source, token for token, and
//               so the same gfx950 code as before the environment map existed;
//   JPT_ENV 1   the *_env kernels (jpt_set_environment): one more parameter, the map (EnvDev, by value), and env_radiance at
//               every miss.  wf2_primary_env queues its misses with its hits, for wf2_shade_env to look up (it takes no map);
//               wf2_accumulate_env makes up every sky-culled pixel exactly, frame by frame: the sky cells bound the gradient only.
//   JPT_ENV 2   the *_mis kernels (jpt_set_environment_sampling, JPT_ENV_SAMPLING_MIS): shade_entry_mis, wf2_shade_mis and
//               wf2_finish_mis, which also take the map's sampling tables (EnvSampDev) and the shadow queue (Wf2Nee).  A vertex
//               below the last bounce draws one map direction (env_nee) and queues a shadow ray for wf2_occlude; a miss at bounce
//               >= 1 is weighted against that strategy (env_miss_weight).  The primary and accumulation launches are the *_env
//               ones: a primary miss has weight 1.
//   JPT_ENV 3   the *_lt kernels (jpt_set_light_sampling, JPT_LIGHT_SAMPLING_MIS): shade_entry_lt, wf2_shade_lt and wf2_finish_lt,
//               which take the emitter tables (LightDev), both shadow queues (Wf2Nee: the map's, the emitters') and the miss model
//               as a run-time value, env_mode: 0 the gradient, 1 the map, 2 the map with JPT_ENV_SAMPLING_MIS.  A vertex below the
//               last bounce queues the map's shadow ray (env_mode 2) and the emitters' (light_nee, bounded by tmax); a hit at
//               bounce >= 1 weighs its emission against the emitter strategy (light_hit_weight).  They pair with the primary and
//               accumulation launches of the miss model in use.
//   JPT_ENV 4   the *_tx kernels (jpt_set_material_extensions, JPT_MATERIAL_EXT_TRANSMISSION over a scene with a transmissive material):
//               shade_entry_tx, wf2_shade_tx and wf2_finish_tx, the general family: the *_lt kernels with emitter sampling on or
//               off at run time (lt.n == 0: no table is read) and the transmission lobe at every hit below the last bounce
//               (transmission_step, jpt_shade.h): a dielectric vertex queues no shadow ray and leaves kDeltaDensity where the
//               BRDF density goes, so the next vertex's weights are 1.  One family for every lighting a glass scene is put under.
// A run-time branch on the map in the default kernels would cost them registers; a template parameter would change their names.
// (No include guard: that is the point.)  Which family a render launches: Lighting::kind, or *_tx with Lighting::transmissive (jpt_kernels.h), decided on the host.
#if JPT_ENV >= 3
#if JPT_ENV == 4
#define JPT_ENV_NAME(name) name##_tx
#define JPT_LTOTAL (lt.n != 0u ? lt.marg[lt.n_blocks] : 0.0f)   // (emitter sampling off: no tables, nothing is read through them)
#define JPT_MISS_WEIGHT env_miss_weight_tx
#define JPT_HIT_WEIGHT light_hit_weight_tx
#else
#define JPT_ENV_NAME(name) name##_lt
#define JPT_LTOTAL lt.marg[lt.n_blocks]
#define JPT_MISS_WEIGHT env_miss_weight
#define JPT_HIT_WEIGHT light_hit_weight
#endif
#define JPT_ENV_PARAM , EnvDev env, EnvSampDev es, LightDev lt, Wf2Nee nee, Wf2Nee lnee, int env_mode
#define JPT_ENV_ARG , env, es, lt, nee, lnee, env_mode
#define JPT_NEE_PARAM , bool& shadow, float4& so, float4& sd, float4& sc4, bool& lshadow, float4& lso, float4& lsd, float4& lsc
#define JPT_NEE_ARG , shadow, so, sd, sc4, lshadow, lso, lsd, lsc
#define JPT_SKY(d) (env_mode != 0 ? env_radiance(env, d) : sample_sky(d))
#define JPT_PDF lnee.pdf
#elif JPT_ENV == 2
#define JPT_ENV_NAME(name) name##_mis
#define JPT_ENV_PARAM , EnvDev env, EnvSampDev es, Wf2Nee nee
#define JPT_ENV_ARG , env, es, nee
#define JPT_NEE_PARAM , bool& shadow, float4& so, float4& sd, float4& sc4
#define JPT_NEE_ARG , shadow, so, sd, sc4
#define JPT_SKY(d) env_radiance(env, d)
#define JPT_PDF nee.pdf
#elif JPT_ENV
#define JPT_ENV_NAME(name) name##_env
#define JPT_ENV_PARAM , EnvDev env
#define JPT_ENV_ARG , env
#define JPT_NEE_PARAM
#define JPT_NEE_ARG
#define JPT_SKY(d) env_radiance(env, d)
#else
#define JPT_ENV_NAME(name) name
#define JPT_ENV_PARAM
#define JPT_ENV_ARG
#define JPT_NEE_PARAM
#define JPT_NEE_ARG
#define JPT_SKY(d) sample_sky(d)
#endif

#if JPT_ENV < 2   // (the MIS and light pipelines run the primary launch of their miss model)

// ---- bounce 0: generate + trace ------------------------------------------------------------------------

// JPT_LENS defined (with JPT_ENV 0 or 1: two more inclusions, of this kernel alone): the lens forms wf2_primary_lens and
// wf2_primary_env_lens (jpt_set_lens) -- the lens (LensDev, by value) where the sky cull was, the thin-lens step (lens_ray,
// jpt_lens.h) after primary_ray, and no cull: a pixel outside the screen rectangles of the root's boxes may still see geometry from
// a point of the aperture.  The body is shared by the preprocessor, like the miss models, and for the same reason: as a
// __forceinline__ template called from both kernels it cost wf2_primary its register allocation (different code, measured on the
// ISA); this way the pinhole kernels' source is what it was, token for token.
//
// JPT_CAMERA_MODEL defined (likewise): the forms wf2_primary_cam and wf2_primary_env_cam (jpt_set_camera_model) -- the model
// (CamModelDev, by value) where the sky cull was, camera_ray (jpt_camera.h) in place of primary_ray, and no cull: the rectangles are
// the pinhole's.  The model is a kernel argument, so the branch between its two recipes is a scalar one.
//
// JPT_BAKE defined (likewise): the forms wf2_primary_bake and wf2_primary_env_bake (jpt_set_bake_texels) -- the texel images
// (BakeDev, by value) where the sky cull was; at refill the lane reads its texel's normal (16 B) and, for a valid texel, its position
// (16 B) and starts the path with bake_ray (jpt_bake.h).  An invalid texel traces nothing: its path ends here with radiance 0 and
// first-hit distance cam.far_, as a sky path of the default kernel ends in save_results, and is not counted as a ray.  No cull.
//
// JPT_PROBE defined (likewise): the forms wf2_primary_probe and wf2_primary_env_probe (jpt_set_probes) -- the probes (ProbeDev, by
// value) where the sky cull was; at refill the lane divides its pixel into (probe, i, j) -- two v_mul_hi_u32 by reciprocals the host
// made, the divisors being kernel arguments -- reads the probe's position (12 B) and starts the path with probe_ray (jpt_probe.h).  A
// pixel of a tile without a probe traces nothing, like an invalid texel.  No cull.
//
// JPT_CUBE defined (likewise): the forms wf2_primary_cube and wf2_primary_env_cube (jpt_set_reflection_probes) -- the reflection
// probes (CubeDev, by value) where the sky cull was; at refill the lane divides its pixel into (probe, face, i, j) -- shifts and masks
// by a kernel argument and one v_mul_hi_u32 for the / 6 --, reads the probe's position (12 B) and starts the path with cube_ray
// (jpt_cube.h).  A pixel of a strip without a probe traces nothing, like an invalid texel.  No cull.
//
// launch_wf2_render takes one of these twelve forms by the kind of the render's PrimaryRays (jpt_kernels.h) and its miss model.
#ifdef JPT_LENS
#if JPT_ENV
#define JPT_PRIMARY_NAME wf2_primary_env_lens
#else
#define JPT_PRIMARY_NAME wf2_primary_lens
#endif
#define JPT_PRIMARY_PARAM LensDev lens
#elif defined(JPT_CAMERA_MODEL)
#if JPT_ENV
#define JPT_PRIMARY_NAME wf2_primary_env_cam
#else
#define JPT_PRIMARY_NAME wf2_primary_cam
#endif
#define JPT_PRIMARY_PARAM CamModelDev cm
#elif defined(JPT_BAKE)
#if JPT_ENV
#define JPT_PRIMARY_NAME wf2_primary_env_bake
#else
#define JPT_PRIMARY_NAME wf2_primary_bake
#endif
#define JPT_PRIMARY_PARAM BakeDev bake
#elif defined(JPT_PROBE)
#if JPT_ENV
#define JPT_PRIMARY_NAME wf2_primary_env_probe
#else
#define JPT_PRIMARY_NAME wf2_primary_probe
#endif
#define JPT_PRIMARY_PARAM ProbeDev probe
#elif defined(JPT_CUBE)
#if JPT_ENV
#define JPT_PRIMARY_NAME wf2_primary_env_cube
#else
#define JPT_PRIMARY_NAME wf2_primary_cube
#endif
#define JPT_PRIMARY_PARAM CubeDev cube
#else
#define JPT_PRIMARY_NAME JPT_ENV_NAME(wf2_primary)
#define JPT_PRIMARY_PARAM SkyCull cull
#endif

template <bool COUNT, bool W4, bool TAIL = false>   // TAIL: the wave finishes its last, long walks itself, all lanes on one ray (coop_walk_call)
__global__ __launch_bounds__(kBlock, JPT_PRIMARY_WAVES) void JPT_PRIMARY_NAME(WideSceneDev sc, Wf2Buffers wb, Wf2Dims dm, FrameParams fp, RefCamera cam,
                                                      WfTune tune, JPT_PRIMARY_PARAM, DevCounters* __restrict__ counters)
{
    __shared__ int32_t stack[kStackLds * kBlock];
    __shared__ uint32_t s_cursor, s_out;
    const int lane = threadIdx.x & 63;
    const uint32_t seg = blockIdx.x;
    // runs seg, seg + G, seg + 2G, ... of 2^run_shift consecutive chunks belong to this block
    const uint32_t run_mask = (1u << dm.run_shift) - 1u;
    const uint32_t n_runs = (dm.n_chunks + run_mask) >> dm.run_shift;
    const uint32_t my_runs = seg < n_runs ? (n_runs - seg + kSegments - 1u) / kSegments : 0u;
    const uint32_t n = (my_runs << dm.run_shift) * 64u;  // (the last run of the image may be short: checked per entry)
    if (threadIdx.x == 0) {
        s_cursor = 0;
        s_out = 0;
    }
    // The queue sizes of bounces >= 1 are accumulated with atomics by wf2_shade and must start from zero: block s clears segment s's
    // word of every later row (and block 0 the set-aside counts behind them) -- this launch completes before the first wf2_shade
    // starts, and one launch fewer per render is one link less in a chain of a dozen (a memset used to do this).
    // (Thread t clears row t, threads 192.. of block 0 the 64 set-aside words: the two ranges must stay apart and inside the block.
    // jpt_set_params refuses max_bounces > kMaxBounces; the same two conditions stand at the carve, wf2_layout.)
    static_assert(kBlock >= 192 + 64, "threads 192 .. 255 of block 0 clear the 64 set-aside words");
    static_assert(kMaxBounces + 1 < 192, "threads 1 .. max_bounces + 1 clear the queue-size rows: they must end below thread 192");
    if ((int)threadIdx.x >= 1 && (int)threadIdx.x <= fp.max_bounces + 1) wb.qcount[(size_t)threadIdx.x * kSegments + seg] = 0u;
    if (seg == 0 && threadIdx.x >= 192u) wb.redo_count[threadIdx.x - 192u] = 0u;
    __syncthreads();
    int32_t spill[kStackSpill];
    const typename Traversal<COUNT, W4>::Stack my_stack{&stack[threadIdx.x], spill, kTraceBlock, kStackLds};
    const size_t seg_base = (size_t)seg * dm.seg_cap;
    uint32_t dry_rounds = 0;   // (TAIL: rounds of this wave since the block's queue ran dry; wave-uniform)
    DevCounters cnt = {};
    Traversal<COUNT, W4> tr;
    bool active = false, exhausted = false;
    bool unsaved = false;   // this lane's finished walk has not left its result yet (see wf2_trace: written when the wave refills)
    uint32_t path = 0;
    uint32_t walk_steps = 0;   // (counting builds: record steps of this lane's ray)
    auto save_results = [&]() {
        // hits are packed into the segment's bounce-0 queue (main.glsl:349), one counter update per wave
#if JPT_ENV
        // (with a map every finished walk is queued, misses too: wf2_shade_env looks them up, exactly as it looks up a later
        // bounce's misses -- the lookup's registers inlined here would cost this kernel spills in its walk)
        const bool is_hit = unsaved;
#else
        const bool is_hit = unsaved && tr.hit.t < 1e9f;
#endif
        const unsigned long long hm = __ballot(is_hit);
        if (hm) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&s_out, (uint32_t)__popcll(hm));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (is_hit) {
                const uint32_t j = base + lanes_below(hm, lane);
                stream_st4(&wb.ray_o[0][seg_base + j], make_float4(tr.wo.x, tr.wo.y, tr.wo.z, 0.0f));
                stream_st4(&wb.ray_d[0][seg_base + j], make_float4(tr.wd.x, tr.wd.y, tr.wd.z, __uint_as_float(path)));
                stream_st4(&wb.hit_a[seg_base + j], make_float4(tr.hit.t, tr.hit.u, tr.hit.v, __uint_as_float(tr.hit.tri)));
                stream_stu(&wb.hit_b[seg_base + j], tr.hit.inst | (tr.hit.front ? 0x80000000u : 0u));
            }
        }
#if !JPT_ENV
        if (unsaved && !is_hit) {   // sky: radiance += 1 * sampleSky(d), path over (main.glsl:380,395-397)
            uint32_t pslot, f;
            path_slot_frame(path, dm, (uint32_t)fp.n_frames, pslot, f);
            const f3 sky = mk3(0.0f, 0.0f, 0.0f) + mk3(1.0f, 1.0f, 1.0f) * JPT_SKY(tr.wd);
            store_final(wb, fp.accum_mode, path, sky);
            if ((int)f == fp.depth_frame) wb.first_depth[pslot] = cam.far_;
        }
#endif
        unsaved = false;
    };

    for (;;) {
        const unsigned long long idle = __ballot(!active);
        const int n_idle = __popcll(idle);
        if (!exhausted && n_idle >= tune.primary_refill_idle) {
            if (__any(unsaved)) save_results();
            uint32_t start = 0;
            if (lane == 0) start = atomicAdd(&s_cursor, (uint32_t)n_idle);
            start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
            if (start + (uint32_t)n_idle >= n) exhausted = true;
            if (start < n && !active) {
                const uint32_t idx = start + lanes_below(idle, lane);
                if (idx < n) {
                    const uint32_t j = idx >> 6;  // local chunk number: run j >> run_shift, position j & run_mask
                    const uint32_t chunk = ((seg + (j >> dm.run_shift) * kSegments) << dm.run_shift) + (j & run_mask);
                    // a wave takes 64 consecutive path ids: chunk c is (tile c / F, part c % F), its lanes the samples part * 64 + lane of that
                    // tile, sample s being frame s % F of the tile's pixel s / F
                    uint32_t slot = 0, f = 0;
                    if (chunk < dm.n_chunks) path_slot_frame(chunk * 64u + (idx & 63u), dm, (uint32_t)fp.n_frames, slot, f);
                    int px, ly;
                    slot_to_pixel(slot, dm, px, ly);
                    if (chunk < dm.n_chunks && px < fp.width && ly < fp.local_rows) {
                        const int py = local_to_global_row(ly, fp);
                        path = slot * (uint32_t)fp.n_frames + f;
                        if (COUNT) cnt.rays++;
                        // a pixel outside the screen rectangles of all the boxes the TLAS root offers: the walk would
                        // expand the root, fail every box test and end in the sky -- nothing is generated, traced or
                        // stored for it here; wf2_accumulate makes up its colour from (x, y, frame)
#ifdef JPT_LENS
                        {
                            uint32_t sx, sy;
                            Ray ray = primary_ray(cam, fp.width, fp.height, px, py, fp.frame_index + f, sx, sy);
                            lens_ray(lens, sx, sy, ray);
#elif defined(JPT_CAMERA_MODEL)
                        {
                            uint32_t sx, sy;
                            const Ray ray = camera_ray(cam, cm, fp.width, fp.height, px, py, fp.frame_index + f, sx, sy);
#elif defined(JPT_BAKE)
                        const size_t texel = (size_t)py * (size_t)fp.width + (size_t)px;
                        const float4 bake_n = bake.normal[texel];
                        if (!bake_texel_valid(bake_n)) {
                            if (COUNT) cnt.rays--;   // (no ray: the count above is taken back)
                            store_final(wb, fp.accum_mode, path, mk3(0.0f, 0.0f, 0.0f));
                            if ((int)f == fp.depth_frame) wb.first_depth[slot] = cam.far_;
                        } else {
                            uint32_t sx, sy;
                            const Ray ray = bake_ray(bake.position[texel], bake_n, px, py, fp.frame_index + f, sx, sy);
#elif defined(JPT_PROBE)
                        uint32_t probe_q, probe_i, probe_j;
                        if (!probe_cell(probe, px, py, probe_q, probe_i, probe_j)) {
                            if (COUNT) cnt.rays--;   // (no ray: the count above is taken back)
                            store_final(wb, fp.accum_mode, path, mk3(0.0f, 0.0f, 0.0f));
                            if ((int)f == fp.depth_frame) wb.first_depth[slot] = cam.far_;
                        } else {
                            // (probe_ray, jpt_probe.h, taken apart)
                            uint32_t sx, sy;
                            float xi0, xi1;
                            probe_draw(px, py, fp.frame_index + f, sx, sy, xi0, xi1);
                            Ray ray;
                            // (the tile's sides enter vector registers here, per refill: as loop invariants their float forms were
                            // hoisted out of the persistent loop into registers of their own, which the walk then spilled)
                            uint32_t tile_w = probe.tile_w(), tile_h = probe.tile_h();
                            asm volatile("" : "+v"(tile_w), "+v"(tile_h));
                            // (where the position's load stands decides what the TAIL instantiation spills: 92 scratch instructions this
                            // way round and 97 the other without a map, 98 and 96 with one -- tests/test_probe_budgets.py holds both)
#if JPT_ENV
                            ray.d = probe_direction(probe_i, probe_j, tile_w, tile_h, xi0, xi1);
                            ray.o = probe_position(probe, probe_q);
#else
                            ray.o = probe_position(probe, probe_q);
                            ray.d = probe_direction(probe_i, probe_j, tile_w, tile_h, xi0, xi1);
#endif
#elif defined(JPT_CUBE)
                        uint32_t cube_q, cube_f, cube_i, cube_j;
                        if (!cube_cell(cube, px, py, cube_q, cube_f, cube_i, cube_j)) {
                            if (COUNT) cnt.rays--;   // (no ray: the count above is taken back)
                            store_final(wb, fp.accum_mode, path, mk3(0.0f, 0.0f, 0.0f));
                            if ((int)f == fp.depth_frame) wb.first_depth[slot] = cam.far_;
                        } else {
                            // (cube_ray, jpt_cube.h, taken apart)
                            uint32_t sx, sy;
                            float xi0, xi1;
                            cube_draw(px, py, fp.frame_index + f, sx, sy, xi0, xi1);
                            Ray ray;
                            // (the face size enters a vector register here, per refill, as the probe forms' tile sides do: as a loop
                            // invariant its float form would be hoisted out of the persistent loop into a register of its own)
                            uint32_t face_size = cube.face_size();
                            asm volatile("" : "+v"(face_size));
                            // (the position's load stands where the probe forms' does, by miss model: with a map and the load first the
                            // TAIL instantiation has one scratch instruction more than the lens forms' budget -- tests/test_reflection_budgets.py)
#if JPT_ENV
                            ray.d = cube_direction(cube_f, cube_i, cube_j, face_size, xi0, xi1);
                            ray.o = cube_position(cube, cube_q);
#else
                            ray.o = cube_position(cube, cube_q);
                            ray.d = cube_direction(cube_f, cube_i, cube_j, face_size, xi0, xi1);
#endif
#else
                        if (sky_culled(cull, px, py)) {
                            if (COUNT) {
                                cnt.tlas_expand++;
                                cnt.phase[7]++;
                            }
                        } else {
                            uint32_t sx, sy;
                            const Ray ray = primary_ray(cam, fp.width, fp.height, px, py, fp.frame_index + f, sx, sy);
#endif
                            tr.begin(sc, ray.o, ray.d);
                            active = true;
                            walk_steps = 0;
                        }
                    }
                }
            }
        }
        if (!__any(active)) {
            if (exhausted) break;
            continue;
        }
        {
            if (walk_round<COUNT, W4>(tr, active, sc, my_stack, cnt, tune, walk_steps)) {
                active = false;
                unsaved = true;
                if (COUNT) count_walk(cnt, walk_steps);
            }
            if constexpr (TAIL && W4) {
                if (exhausted && ++dry_rounds >= (uint32_t)tune.tail_rounds && __popcll(__ballot(active)) <= tune.tail_lanes) break;
            }
        }
    }
    if constexpr (TAIL && W4) {
        // tail phase (coop_walk_call): the few rays this wave still holds, each walked by the whole wave
        unsigned long long left = __ballot(active);
        if (left) {
            if (__any(unsaved)) save_results();   // (the finished lanes' hits leave the registers the call is free to use)
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
                    active = false;
                    unsaved = true;
                }
            }
        }
    }
    if (__any(unsaved)) save_results();
    __syncthreads();
    if (threadIdx.x == 0) wb.qcount[0 * kSegments + seg] = s_out;
    if (COUNT) flush_counters(cnt, counters);
}

#undef JPT_PRIMARY_NAME
#undef JPT_PRIMARY_PARAM
#endif  // JPT_ENV < 2

#if !defined(JPT_LENS) && !defined(JPT_CAMERA_MODEL) && !defined(JPT_BAKE) && !defined(JPT_PROBE) && !defined(JPT_CUBE)   // (everything below: once per miss model)

// ---- shading: one path vertex per queue entry (main.glsl:378-397) -------------------------------------------

#ifndef JPT_SHADE_WAVES
#define JPT_SHADE_WAVES 5   // 96 VGPRs: two fewer than the body wants, five waves per SIMD instead of four for a kernel that waits on gathers (C3 +4 %); 6 spills
#endif
// One path vertex (main.glsl:378-397): the queue entry's ray and closest hit in, radiance / throughput / seeds of the path
// updated, returns true when the path goes on (no / nd = its next ray).  With reach records (JPT_BUILD_SAH) and
// check_reach, a hit the reference's own traversal could not have reached -- the world ray fails the world box the
// reference gives the instance, or the local ray fails the box of the triangle's reference leaf (jpt_types.h) -- is
// not shaded: the vertex is set aside (redo_rec; its state parked in the path's thr / rad words), `unreachable` comes back
// true, and the path leaves the wavefront to be finished by wf2_finish.
// LAST: the vertex is known to be the path's last (bounce == max_bounces): emission or sky is added and the path ends -- no BRDF
// sample, no next ray -- so the instantiation carries none of that code (wf2_shade's final launch).
template <bool COUNT, bool LAST = false, int TEX = 3>
__device__ __forceinline__ bool JPT_ENV_NAME(shade_entry)(const SceneShading& sh, const Wf2Buffers& wb, const Wf2Dims& dm, const FrameParams& fp, float cam_far,
                                            int bounce, const float4 ro, const float4 rd, const float4 tin, const float4 ha, const uint32_t hb,
                                            bool check_reach, bool& unreachable, float4& no, float4& nd, float4& nt, DevCounters& cnt JPT_ENV_PARAM JPT_NEE_PARAM)
{
    unreachable = false;
#if JPT_ENV == 2
    // (MIS: a shadow ray of this vertex, for wf2_occlude: so = origin.xyz | path id + kNeeFinal when the path ends here, sd = the map
    // direction, sc4 = the contribution if unoccluded.  rad[path] then holds the radiance so far, which the shadow ray adds to.)
    shadow = false;
#elif JPT_ENV >= 3
    // (lights: the map's shadow ray as above when env_mode is 2, and the emitters' in lso / lsd (direction, tmax) / lsc; when both
    // are cast the map's lands first, and the one that lands last stores a path that ends here)
    shadow = false;
    lshadow = false;
#endif
    const uint32_t p = __float_as_uint(rd.w) & kPathMask;
    const bool had_radiance = (__float_as_uint(rd.w) & kHasRadiance) != 0u;
    f3 throughput, radiance;
    uint32_t sx, sy;
    uint32_t slot, f;
    path_slot_frame(p, dm, (uint32_t)fp.n_frames, slot, f);
    Ray ray;
    ray.o = mk3(ro.x, ro.y, ro.z);
    ray.d = mk3(rd.x, rd.y, rd.z);
    const bool is_hit = ha.x < 1e9f;  // main.glsl:349
    // The kernel waits on gathers, so everything whose address is known once the queue entry is here is asked for at
    // once, ahead of the branches that use it: the path's state now, the instance and the reach boxes below.
    const float4 t4 = tin;   // (the entry's throughput and seed.x: came with the ray)
    float4 r4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bounce > 0 && had_radiance) r4 = wb.rad[p];
    Hit h;
    ShadeTriRegs stri;
    uint32_t found_in = 0;
    if (is_hit) {
        h.t = ha.x;
        h.u = ha.y;
        h.v = ha.z;
        h.tri = __float_as_uint(ha.w);
        h.inst = hb & kInstMask;                   // hitInfo.blas
        found_in = (hb >> kInstBits) & kInstMask;  // the instance whose local ray found the triangle
        const bool check = check_reach && sh.reach_tri != nullptr;
        stri = load_shade_tri(sh, h.tri);
        float4 ta, tb, ia, ib;
        if (check) {   // (whole records, unconditionally: a flag test first would put two round trips in a row)
            ta = ld4(&sh.reach_tri[h.tri].lo[0]);
            tb = ld4(&sh.reach_tri[h.tri].hi[0]);
            if (sh.n_instances > 1u) {
                ia = ld4(&sh.reach_inst[found_in].lo[0]);
                ib = ld4(&sh.reach_inst[found_in].hi[0]);
            }
        }
        // the hit instance's local ray: the expression ray_trace_tlas evaluates (main.glsl:319-320)
        const RefInstance& b = sh.instances[found_in];
        h.lo = xform_point(b.inverse_transform, ray.o);
        h.ld = xform_dir(b.inverse_transform, ray.d);
        if (check) {
            bool reached = __float_as_uint(ta.w) != 0u || slab(h.lo, rcp3(h.ld), ta.x, ta.y, ta.z, tb.x, tb.y, tb.z) < 1e30f;
            if (reached && sh.n_instances > 1u) reached = slab(ray.o, rcp3(ray.d), ia.x, ia.y, ia.z, ib.x, ib.y, ib.z) < 1e30f;
            // (an exact distance tie is as undecidable on the native tree as a crack: with the reference's trees at hand
            // it is decided where the reference decides it)
            if (sh.retrace_ties && (hb & kHitTied) != 0u) reached = false;
            if (!reached) {
                // a few paths in 10^7: the path leaves the wavefront here and is finished, exactly, by wf2_finish -- unless
                // the set-aside buffer is full (pathological scenes): then the hit is shaded as found, and counted
                const uint32_t k = atomicAdd(&wb.redo_count[0], 1u);
                if (k < wb.redo_cap) {
                    float4 rd2 = rd;
                    if (bounce > 0) {   // its seed.y (the entry's origin.w) waits in rad[path].w, beside the radiance so far
                        wb.rad[p] = make_float4(r4.x, r4.y, r4.z, ro.w);
                        wb.thr[p] = tin;
                        rd2.w = __uint_as_float(p | kHasRadiance);
                    }
                    wb.redo_rec[2 * (size_t)k] = make_float4(ro.x, ro.y, ro.z, __uint_as_float((uint32_t)bounce));
                    wb.redo_rec[2 * (size_t)k + 1] = rd2;
                    unreachable = true;
                    return false;
                }
                atomicAdd(&wb.redo_count[1], 1u);
            }
        }
    }
    if (bounce == 0) {
        // fresh path: the seed after the jitter draw (main.glsl:409-411), recomputed from (x, y, frame)
        int px, ly;
        slot_to_pixel(slot, dm, px, ly);
        prng_seed((uint32_t)px, (uint32_t)local_to_global_row(ly, fp), fp.frame_index + f, sx, sy);
        float r0, r1;
        pcg2d(sx, sy, r0, r1);
        throughput = mk3(1.0f, 1.0f, 1.0f);
        radiance = mk3(0.0f, 0.0f, 0.0f);
    } else {
        throughput = mk3(t4.x, t4.y, t4.z);
        radiance = mk3(r4.x, r4.y, r4.z);
        sx = __float_as_uint(t4.w);
        sy = __float_as_uint(ro.w);
    }
    const f3 radiance_in = radiance;
    if (COUNT && bounce > 0) cnt.rays++;
    bool alive = false;
    if (!is_hit) {
#if JPT_ENV == 2
        if (bounce > 0) radiance = radiance + (throughput * JPT_SKY(ray.d)) * env_miss_weight(env, es, ray.d, nee.pdf[p]);
        else
#elif JPT_ENV >= 3
        if (bounce > 0 && env_mode == 2) radiance = radiance + (throughput * JPT_SKY(ray.d)) * JPT_MISS_WEIGHT(env, es, ray.d, lnee.pdf[p]);
        else
#endif
        radiance = radiance + throughput * JPT_SKY(ray.d);
        if (bounce == 0 && (int)f == fp.depth_frame) wb.first_depth[slot] = cam_far;  // (only a redone primary hit can turn into a miss here)
    } else {
        if (COUNT) cnt.shaded_hits++;
        const Shading s = get_shading_data<TEX>(sh, h, (hb >> 31) != 0u, stri);
#if JPT_ENV >= 3
        const float ltotal = JPT_LTOTAL;
        if (bounce > 0) radiance = radiance + (throughput * s.emission) * JPT_HIT_WEIGHT(lt, ltotal, sh, h, s, ray.o, ray.d, lnee.pdf + p);
        else
#endif
        radiance = radiance + throughput * s.emission;
        if (bounce == 0 && (int)f == fp.depth_frame) wb.first_depth[slot] = length3(s.position - ray.o);
#if JPT_ENV >= 2
        if (!LAST && bounce < fp.max_bounces) {
#if JPT_ENV == 4
          // (the transmission lobe: a dielectric vertex casts no shadow ray, never ends the path and leaves the sentinel density)
          if (transmission_step(s, material_ext<TEX>(sh, h, stri), (hb >> 31) != 0u, sx, sy, ray, throughput)) {
            alive = true;
            JPT_PDF[p] = kDeltaDensity;
          } else {
#endif
#if JPT_ENV >= 3
          if (env_mode == 2) {
#endif
            f3 l, c;
            shadow = env_nee(s, env, es, sx, sy, throughput, l, c);
            if (shadow) {
                const f3 so3 = s.position + s.normal * 0.001f;
                so = make_float4(so3.x, so3.y, so3.z, __uint_as_float(p));
                sd = make_float4(l.x, l.y, l.z, 0.0f);
                sc4 = make_float4(c.x, c.y, c.z, 0.0f);
            }
#if JPT_ENV >= 3
          }
            if (ltotal > 0.0f) {
                f3 lo3, ll, lc;
                float tmax;
                lshadow = light_nee(s, lt, ltotal, sx, sy, throughput, lo3, ll, tmax, lc);
                if (lshadow) {
                    lso = make_float4(lo3.x, lo3.y, lo3.z, __uint_as_float(p));
                    lsd = make_float4(ll.x, ll.y, ll.z, tmax);
                    lsc = make_float4(lc.x, lc.y, lc.z, 0.0f);
                }
            }
#endif
            float density;
            alive = bounce_step_pdf(s, sx, sy, ray, throughput, density);
            if (alive) JPT_PDF[p] = density;
#if JPT_ENV == 4
          }
#endif
        }
#else
        if (!LAST && bounce < fp.max_bounces) alive = bounce_step(s, sx, sy, ray, throughput);
#endif
        if (COUNT && alive && throughput.x == 0.0f && throughput.y == 0.0f && throughput.z == 0.0f) cnt.zero_thr++;
    }
    if (alive) {
        // (radiance starts as +0 and +0 + x is x or +0, never -0: "unchanged and never written" means exactly +0)
#if JPT_ENV >= 3
        const bool changed = shadow || lshadow || radiance.x != radiance_in.x || radiance.y != radiance_in.y || radiance.z != radiance_in.z;
#elif JPT_ENV == 2
        const bool changed = shadow || radiance.x != radiance_in.x || radiance.y != radiance_in.y || radiance.z != radiance_in.z;
#else
        const bool changed = radiance.x != radiance_in.x || radiance.y != radiance_in.y || radiance.z != radiance_in.z;
#endif
        if (changed) wb.rad[p] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
        nt = make_float4(throughput.x, throughput.y, throughput.z, __uint_as_float(sx));
        no = make_float4(ray.o.x, ray.o.y, ray.o.z, __uint_as_float(sy));
        nd = make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(p | ((had_radiance || changed) ? kHasRadiance : 0u)));
    } else {
#if JPT_ENV == 2
        if (shadow) {   // the path ends here, but its shadow ray has yet to land: wf2_occlude stores its final value
            wb.rad[p] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
            so.w = __uint_as_float(p | kNeeFinal);
        } else
#elif JPT_ENV >= 3
        if (shadow || lshadow) {   // the path ends here: the shadow ray that lands last (the emitters') stores its final value
            wb.rad[p] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
            if (lshadow) lso.w = __uint_as_float(p | kNeeFinal);
            else so.w = __uint_as_float(p | kNeeFinal);
        } else
#endif
        store_final(wb, fp.accum_mode, p, radiance);
    }
    return alive;
}

#ifndef JPT_SHADE_NOTEX_WAVES
#define JPT_SHADE_NOTEX_WAVES 7   // without the sampler code the body takes 67 VGPRs by itself
#endif
template <bool COUNT, bool LAST = false, int TEX = 3>
__global__ __launch_bounds__(kBlock, LAST ? 8 : (TEX == 0 ? JPT_SHADE_NOTEX_WAVES : JPT_SHADE_WAVES)) void JPT_ENV_NAME(wf2_shade)(SceneShading sh, Wf2Buffers wb, Wf2Dims dm, FrameParams fp, float cam_far, int bounce,
                                                    DevCounters* __restrict__ counters JPT_ENV_PARAM)
{
    // grid = (chunks per segment, segments): every 256-entry chunk of every segment is its own block, so the
    // launch is balanced however unevenly the segments are filled; blocks past a segment's end exit at once.
    const int lane = threadIdx.x & 63;
    const uint32_t seg = blockIdx.y;
    const uint32_t n = wb.qcount[(size_t)bounce * kSegments + seg];
    const uint32_t base = blockIdx.x * kBlock;
    if (base >= n) return;
    const size_t seg_base = (size_t)seg * dm.seg_cap;
    const int in = bounce & 1, out = (bounce + 1) & 1;
    DevCounters cnt = {};
    const uint32_t i = base + threadIdx.x;
    bool alive = false;
    float4 no, nd, nt;
#if JPT_ENV >= 2
    bool shadow = false;
    float4 so, sd, sc4;
#endif
#if JPT_ENV >= 3
    bool lshadow = false;
    float4 lso, lsd, lsc;
#endif
    if (i < n) {
        const float4 ro = stream_ld4(&wb.ray_o[in][seg_base + i]), rd = stream_ld4(&wb.ray_d[in][seg_base + i]);
        const float4 tin = bounce > 0 ? stream_ld4(&wb.thr_q[in][seg_base + i]) : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        const float4 ha = stream_ld4(&wb.hit_a[seg_base + i]);
        const uint32_t hb = stream_ldu(&wb.hit_b[seg_base + i]);
        bool unreachable;   // (set aside inside shade_entry: nothing more to do here)
        alive = JPT_ENV_NAME(shade_entry)<COUNT, LAST, TEX>(sh, wb, dm, fp, cam_far, bounce, ro, rd, tin, ha, hb, true, unreachable, no, nd, nt, cnt JPT_ENV_ARG JPT_NEE_ARG);
    }
#if JPT_ENV >= 2
    if (!LAST) {   // the shadow rays, packed into the segment's shadow queue of this bounce as the next rays are below
        const unsigned long long sm = __ballot(shadow);
        if (sm) {
            uint32_t sbase = 0;
            if (lane == 0) sbase = atomicAdd(&nee.scount[(size_t)bounce * kSegments + seg], (uint32_t)__popcll(sm));
            sbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)sbase);
            if (shadow) {
                const size_t j = seg_base + sbase + lanes_below(sm, lane);
                stream_st4(&nee.sh_o[j], so);
                stream_st4(&nee.sh_d[j], sd);
                stream_st4(&nee.sh_c[j], sc4);
            }
        }
    }
#endif
#if JPT_ENV >= 3
    if (!LAST) {   // the emitters' shadow rays, into their own queue (traced after the map's: the two never share a launch)
        const unsigned long long lm = __ballot(lshadow);
        if (lm) {
            uint32_t lbase = 0;
            if (lane == 0) lbase = atomicAdd(&lnee.scount[(size_t)bounce * kSegments + seg], (uint32_t)__popcll(lm));
            lbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)lbase);
            if (lshadow) {
                const size_t j = seg_base + lbase + lanes_below(lm, lane);
                stream_st4(&lnee.sh_o[j], lso);
                stream_st4(&lnee.sh_d[j], lsd);
                stream_st4(&lnee.sh_c[j], lsc);
            }
        }
    }
#endif
    if (LAST) {   // (no path goes on: nothing to pack)
        if (COUNT) flush_counters(cnt, counters);
        return;
    }
    // active-ray packing: wave ballot + prefix popcount, one atomic per wave on the SEGMENT's counter (1792
    // different words: no hot address); the order inside the next queue is irrelevant
    const unsigned long long m = __ballot(alive);
    if (m) {
        uint32_t wbase = 0;
        if (lane == 0) wbase = atomicAdd(&wb.qcount[(size_t)(bounce + 1) * kSegments + seg], (uint32_t)__popcll(m));
        wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        if (alive) {
            const size_t j = seg_base + wbase + lanes_below(m, lane);
            stream_st4(&wb.ray_o[out][j], no);
            stream_st4(&wb.ray_d[out][j], nd);
            stream_st4(&wb.thr_q[out][j], nt);
        }
    }
    if (COUNT) flush_counters(cnt, counters);
}

// The paths wf2_shade set aside: their hit is one the reference's traversal cannot reach.  Each is finished here, after
// the render's last bounce launch and before the accumulation: from the vertex where it left the wavefront the path is
// traced with the reach tests applied to every instance entry and every accepted triangle (Traversal<.., REACH = true>:
// the closest hit among the triangles the reference can reach, i.e. the reference's answer) and shaded bounce after
// bounce by the same shade_entry, its state passing through the path's own thr / rad words.  A handful of paths per
// render, so one small grid of single-wave blocks with the whole stack in scratch; one launch per render.
template <bool COUNT, bool W4, bool EXACT>
__global__ __launch_bounds__(64) void JPT_ENV_NAME(wf2_finish)(WideSceneDev sc, TieShadowDev sx, SceneShading sh, Wf2Buffers wb, Wf2Dims dm, FrameParams fp, float cam_far,
                                                 DevCounters* __restrict__ counters JPT_ENV_PARAM)
{
    const uint32_t n = wb.redo_count[0] < wb.redo_cap ? wb.redo_count[0] : wb.redo_cap;
    if (blockIdx.x >= n) return;
    constexpr int kDepth = kStackLds + kStackSpill;
    int32_t stack_mem[kDepth];   // (the whole stack in scratch; in LDS instead: no difference, profiles/r03/r03z_finish_probe.txt)
    // Every segment of a set-aside path is traced on the native tree with the two reach tests applied inside the walk: the
    // closest hit among the triangles the reference can reach.  EXACT (`sx` = the reference's own trees): when that walk
    // met a second reachable triangle at exactly the closest distance, the tie is decided where the reference decides it
    // (jpt_tie_walk.h).
    using Walk = Traversal<COUNT, W4, true>;
    const typename Walk::Stack st{nullptr, stack_mem, 0, 0, kDepth};
    DevCounters cnt = {};
    // (records are dealt to the BLOCKS first -- record k to block k % grid, lane k / grid: a handful of set-aside paths run as
    // one lane each of as many waves, side by side, instead of as divergent lanes of one wave, one after another)
    for (uint32_t k = threadIdx.x * gridDim.x + blockIdx.x; k < n; k += gridDim.x * 64u) {
        float4 ro = wb.redo_rec[2 * (size_t)k], rd = wb.redo_rec[2 * (size_t)k + 1];
        const int first = (int)__float_as_uint(ro.w);
        float4 tin = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        if (first > 0) {   // the seed.y and the throughput parked when the path was set aside
            ro.w = wb.rad[__float_as_uint(rd.w) & kPathMask].w;
            tin = wb.thr[__float_as_uint(rd.w) & kPathMask];
        }
        for (int bounce = first;; bounce++) {
            const f3 o3 = mk3(ro.x, ro.y, ro.z), d3 = mk3(rd.x, rd.y, rd.z);
            Walk tr;
            tr.begin(sc, o3, d3);
            while (tr.step(sc, st, cnt)) {
            }
            TraceHit hit = tr.hit;
            if (EXACT && hit.t < 1e9f && (hit.inst & kHitTied) != 0u) {
                TieLeaves tl;
                tie_leaves<COUNT, W4>(sc, sx, st, o3, d3, hit.t, tl, cnt);
                TraceHit xh;
                if (tl.n > 0 && tie_walk(sx, sh.instances, sx.tlas_current, tl, o3, d3, xh) && xh.t == hit.t) {
                    // (xh.t differs only if a float accident kept the reference's walk from the tying leaves: then the native
                    // walk's answer stands)
                    hit = xh;
                    hit.tri = sx.tri_native[xh.tri];   // shading and reach records are in the native order
                }
            }
            // (the ray-segment count the host reads is the sum of the queue sizes: this path's later segments are in no queue)
            if (bounce > first) atomicAdd(&wb.qcount[(size_t)bounce * kSegments], 1u);
            const float4 ha = make_float4(hit.t, hit.u, hit.v, __uint_as_float(hit.tri));
            const uint32_t hb = (hit.inst & ~kHitTied) | (hit.front ? 0x80000000u : 0u);
            bool unreachable;
            float4 no, nd, nt;
#if JPT_ENV == 2
            bool shadow;
            float4 so, sd, sc4;
            const bool alive = shade_entry_mis<COUNT>(sh, wb, dm, fp, cam_far, bounce, ro, rd, tin, ha, hb, false, unreachable, no, nd, nt, cnt JPT_ENV_ARG JPT_NEE_ARG);
            if (shadow) {   // the shadow ray at once, on the native tree without reach tests (wf2_occlude's walk)
                Traversal<COUNT, W4> occ;
                const typename Traversal<COUNT, W4>::Stack ost{nullptr, stack_mem, 0, 0, kDepth};
                occ.begin(sc, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z));
                while (occ.hit.t >= 1e9f && occ.step(sc, ost, cnt)) {
                }
                nee_land(wb, fp.accum_mode, so, sc4, occ.hit.t < 1e9f);
            }
            if (!alive) break;
#elif JPT_ENV >= 3
            bool shadow, lshadow;
            float4 so, sd, sc4, lso, lsd, lsc;
            const bool alive = JPT_ENV_NAME(shade_entry)<COUNT>(sh, wb, dm, fp, cam_far, bounce, ro, rd, tin, ha, hb, false, unreachable, no, nd, nt, cnt JPT_ENV_ARG JPT_NEE_ARG);
            if (shadow) {   // the map's shadow ray at once (wf2_occlude's walk), then the emitters' (wf2_occlude_lt's, bounded by tmax)
                Traversal<COUNT, W4> occ;
                const typename Traversal<COUNT, W4>::Stack ost{nullptr, stack_mem, 0, 0, kDepth};
                occ.begin(sc, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z));
                while (occ.hit.t >= 1e9f && occ.step(sc, ost, cnt)) {
                }
                nee_land(wb, fp.accum_mode, so, sc4, occ.hit.t < 1e9f);
            }
            if (lshadow) {
                Traversal<COUNT, W4> occ;
                const typename Traversal<COUNT, W4>::Stack ost{nullptr, stack_mem, 0, 0, kDepth};
                occ.begin(sc, mk3(lso.x, lso.y, lso.z), mk3(lsd.x, lsd.y, lsd.z));
                occ.hit.t = lsd.w;
                while (occ.hit.t >= lsd.w && occ.step(sc, ost, cnt)) {
                }
                nee_land(wb, fp.accum_mode, lso, lsc, occ.hit.t < lsd.w);
            }
            if (!alive) break;
#else
            if (!JPT_ENV_NAME(shade_entry)<COUNT>(sh, wb, dm, fp, cam_far, bounce, ro, rd, tin, ha, hb, false, unreachable, no, nd, nt, cnt JPT_ENV_ARG)) break;
#endif
            ro = no;
            rd = nd;
            tin = nt;
        }
    }
    if (COUNT) flush_counters(cnt, counters);
}

#if JPT_ENV < 2
// ---- per pixel: frames in order -> accumulation buffer, display image, depth ----------------------------------

__global__ __launch_bounds__(kBlock) void JPT_ENV_NAME(wf2_accumulate)(Wf2Buffers wb, Wf2Dims dm, FrameParams fp, RefCamera cam, SkyCull cull,
                                                         float4* __restrict__ accum, uint32_t* __restrict__ ldr,
                                                         float* __restrict__ depth_out, const uint32_t* __restrict__ tile_cell JPT_ENV_PARAM)
{
    // one thread per pixel of the context's share of the image, tile by tile (a wave = one 8 x 8 tile); `slot` is the
    // pixel's place in the window
    constexpr int kSharedFrames = 16;                       // most frames per render the shared exact route below holds
    __shared__ uint32_t s_who[kBlock / 64][64];            // per wave: the pixels that need it, px | py << 16
    __shared__ uint32_t s_val[kBlock / 64][64 * kSharedFrames];   // ... and their frames' rgba8 sky values
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t full_slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t ftile = full_slot >> 6, flane = full_slot & 63u;
    const uint32_t fty = fdiv(ftile, dm.by_full_tiles_x), ftx = ftile - fty * (uint32_t)dm.full_tiles_x;
    if ((int)fty >= dm.full_tiles_y) return;   // (the whole wave)
    const int px = (int)(ftx * 8u + (flane & 7u)), ly = (int)(fty * 8u + (flane >> 3));
    const bool valid = px < fp.width && ly < fp.local_rows;   // (lanes past the image's edge still help with the shared route)
    const int wtx = (int)ftx - dm.tile_x0, wty = (int)fty - dm.tile_y0;
    const bool in_window = wtx >= 0 && wtx < dm.tiles_x && wty >= 0 && wty < dm.tiles_y;
    const uint32_t in_tile = flane;
    const uint32_t slot = in_window ? ((uint32_t)wty * (uint32_t)dm.tiles_x + (uint32_t)wtx) * 64u + in_tile : 0u;
    const size_t idx = valid ? (size_t)ly * fp.width + px : 0;
    // fp.frame_count = ProgressiveRendering frame_count of the FIRST frame of this render
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    bool have_prev = fp.frame_count > 1;
    if (have_prev && valid) {
        const float4 prev = stream_ld4(&accum[idx]);
        sum = mk3(prev.x, prev.y, prev.z);
    }
    f3 last = mk3(0.0f, 0.0f, 0.0f);
    // the primary launch neither traced nor stored the paths of a sky-culled pixel: their radiance is the sky along the
    // primary ray of (x, y, frame) (main.glsl:380,395-397 with throughput 1), made up here
    const int py = local_to_global_row(ly, fp);
    const bool culled = valid && (!in_window || sky_culled(cull, px, py));
    // A culled pixel's frames all see the sky, whose colour depends on the ray's d.y alone and changes by a hundredth of an
    // rgba8 step across a pixel: in REF_LDR8 mode nearly every pixel has ONE rgba8 sky value for all its frames.  The
    // jittered sample of a frame lies on the quarter circle (px + cos, py + sin), inside the pixel's square.  A pinhole
    // maps raster lines to great circles, so the directions through the square fill the spherical quadrilateral of its four
    // corner rays, and along a great circle d.y = A cos(s + phi): f'' = -f.  Every point of the quadrilateral lies on an
    // arc between two points of its edges, so d.y leaves the range of the four corner values by at most
    //     2 * (theta^2 / 8) * max |d.y|        (theta: the quadrilateral's diameter; two levels of interpolation)
    // -- nothing for the narrow pixels of the benchmark cameras (1e-6), but NOT nothing for a wide lens looking at the
    // zenith, where d.y has its maximum INSIDE the square (0.06 of a cell for an 8 x 8 tile at fov 150).  The
    // corner range is therefore widened by that bound, in cell units (d value / d d.y <= 255 * 0.05 * 0.5 = 6.4,
    // main.glsl:189-192), before it is asked to lie inside ONE integer cell of value * 255 + 0.5, `kCellMargin` away from
    // the cell's ends (float rounding of the ray set-up: 1e-5 of a cell); a quadrilateral wider than half a radian is not
    // tried.  When that holds every frame quantises to that cell and the eight primary rays -- seed, sincos, 4 x 4
    // transform, three divisions, a normalisation each -- need not be made.  Pixels near a cell boundary (a few per cent:
    // horizontal bands) and cameras whose clip-space w changes sign inside the pixel take the exact per-frame route below.
    bool sky_constant = false;
    f3 sky_value = mk3(0.0f, 0.0f, 0.0f);
    uint32_t sky_word = 0u;   // ... as the rgba8 word it is converted from
    const float two_over_w = 2.0f / (float)fp.width, two_over_h = 2.0f / (float)fp.height;
    const bool want_cells = !JPT_ENV && fp.accum_mode == 0 && fp.n_frames > 1;
    // First for the whole TILE at once (a wave is one 8 x 8 tile, eight consecutive image rows): do its four corner rays agree on the
    // cells?  Then every culled pixel of the tile has that value.  (The same argument over eight pixels instead of one; theta is
    // eight times larger, so wide lenses fail here and pass pixel by pixel.)  Decided by wf2_sky_tiles, one lane per tile, while
    // the render's paths were traced: here one word per wave.
    bool tile_constant = false;
    if (want_cells && tile_cell != nullptr && __any(culled)) {
        const uint32_t tc = tile_cell[__builtin_amdgcn_readfirstlane((int)ftile)];
        if (tc & 0x80000000u) {
            tile_constant = true;
            if (culled) {
                sky_constant = true;
                sky_word = tc & 0xffffffu;
                sky_value = mk3(from_unorm8(tc & 255u), from_unorm8((tc >> 8) & 255u), from_unorm8((tc >> 16) & 255u));
            }
        }
    }
    // ... then, in the tiles that straddle a cell boundary, pixel by pixel.  (Sharing the tile's 9 x 9 corners through LDS -- two
    // passes of the set-up instead of four -- left the kernel at 49.5 us and cost queued renders 1-5 %: profiles/r04/r04ak_acc_corners.txt)
    if (culled && want_cells && !tile_constant) {
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        bool sane = true;
        float w_first = 1.0f;
        f3 cd[4];
        for (int corner = 0; corner < 4; corner++) {
            float ww, v[3];
            const bool ok = sky_cells_at(cam, two_over_w, two_over_h, (float)(px + (corner & 1)), (float)(py + (corner >> 1)), w_first, ww, v, cd[corner]);
            if (corner == 0) w_first = ww;
            sane = sane && (corner == 0 ? (ww == ww) : ok);
            for (int k = 0; k < 3; k++) {
                lo[k] = fmin_(lo[k], v[k]);
                hi[k] = fmax_(hi[k], v[k]);
            }
        }
        const float excess = sky_interior_excess(cd);
        bool same = sane;
        float cell[3];
        for (int k = 0; k < 3; k++) {
            lo[k] -= excess;
            hi[k] += excess;
            cell[k] = __builtin_floorf(lo[k]);
            same = same && (lo[k] - cell[k] >= kCellMargin) && (hi[k] - cell[k] <= 1.0f - kCellMargin) && (hi[k] - lo[k] < 0.5f);
        }
        if (same) {
            sky_constant = true;
            sky_word = ((uint32_t)cell[0] & 255u) | (((uint32_t)cell[1] & 255u) << 8) | (((uint32_t)cell[2] & 255u) << 16);
            sky_value = mk3(from_unorm8(sky_word & 255u), from_unorm8((sky_word >> 8) & 255u), from_unorm8((sky_word >> 16) & 255u));
        }
    }
    // The culled pixels that did not pass (near a cell boundary) need their frames' exact values -- eight primary rays
    // each.  A wave runs that code for all 64 lanes as soon as ONE pixel of its tile needs it, frame after frame; instead
    // the tile's (pixel, frame) pairs that need it are dealt to the wave's 64 lanes, one pair each, so a tile with eight
    // such pixels makes one pass (64 pairs), not eight.  The values go through LDS to the pixel that sums them, in frame
    // order.  (REF_LDR8, 2..kSharedFrames frames per render; otherwise every lane walks its own frames, as before.)
    const bool shared_route = fp.accum_mode == 0 && fp.n_frames > 1 && fp.n_frames <= kSharedFrames;
    const bool slow = culled && !sky_constant && shared_route;
    uint32_t my_rank = 0;
    {
        const unsigned long long sm = __ballot(slow);
        if (sm) {
            my_rank = lanes_below(sm, lane);
            if (slow) s_who[wave][my_rank] = (uint32_t)px | ((uint32_t)py << 16);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t total = (uint32_t)__popcll(sm) * (uint32_t)fp.n_frames;
            for (uint32_t base = 0; base < total; base += 64u) {
                const uint32_t item = base + (uint32_t)lane;
                if (item < total) {
                    const uint32_t p = fdiv(item, dm.by_frames), f = item - p * (uint32_t)fp.n_frames;
                    const uint32_t who = s_who[wave][p];
                    uint32_t sx, sy;
                    const Ray ray = primary_ray(cam, fp.width, fp.height, (int)(who & 0xffffu), (int)(who >> 16), fp.frame_index + f, sx, sy);
                    const f3 c = mk3(0.0f, 0.0f, 0.0f) + mk3(1.0f, 1.0f, 1.0f) * JPT_SKY(ray.d);
                    s_val[wave][item] = unorm8(c.x) | (unorm8(c.y) << 8) | (unorm8(c.z) << 16);   // rgba8 store of main.glsl:434
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (!valid) return;
    // the frames of group g are a block of their own in rad / fin8: [slot][frame of the group] behind the earlier groups' blocks
    const int g_base = fp.n_frames / dm.acc_groups, g_extra = fp.n_frames % dm.acc_groups;
    int g = 0, g_f0 = 0, g_nf = g_base + (g_extra > 0 ? 1 : 0);
    // The usual case first -- rgba8 samples, one frame group, 4 / 8 / 12 / 16 frames: a pixel's frames are 16 to 64 consecutive bytes of
    // fin8, fetched as one to four 16-byte loads that are all in flight together.  (The loop below waits for a 4-byte load per frame,
    // eight trips to the cache one after another: the kernel was bound by that latency, not by its 53 MB -- round 5.)
    const bool packed_frames = fp.accum_mode == 0 && dm.acc_groups == 1 && fp.n_frames >= 4 && fp.n_frames <= kSharedFrames && (fp.n_frames & 3) == 0;
    if (packed_frames) {
        // every lane's frames as rgba8 words first -- the window's pixels from fin8, a culled pixel's from its one sky cell or from
        // the wave's shared exact values -- then ONE conversion-and-add per frame for all of them
        uint4 q[kSharedFrames / 4];
        const uint4* mine = reinterpret_cast<const uint4*>(wb.fin8 + (size_t)slot * (size_t)fp.n_frames);
        const uint4* shared = reinterpret_cast<const uint4*>(&s_val[wave][my_rank * (uint32_t)fp.n_frames]);
#pragma unroll
        for (int c = 0; c < kSharedFrames / 4; c++) {
            q[c] = make_uint4(sky_word, sky_word, sky_word, sky_word);
            if (c * 4 < fp.n_frames) {
                if (!culled) q[c] = stream_ldu4(&mine[c]);
                else if (slow) q[c] = shared[c];
            }
        }
#pragma unroll
        for (int c = 0; c < kSharedFrames / 4; c++) {
            if (c * 4 >= fp.n_frames) break;
            const uint32_t qs[4] = {q[c].x, q[c].y, q[c].z, q[c].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const f3 cur = mk3(from_unorm8(qs[j] & 255u), from_unorm8((qs[j] >> 8) & 255u), from_unorm8((qs[j] >> 16) & 255u));
                last = cur;
                sum = have_prev ? cur + sum : cur;  // progressive_rendering.glsl:34-36
                have_prev = true;
            }
        }
    }
    for (int f = 0; f < fp.n_frames && !packed_frames; f++) {
        if (f >= g_f0 + g_nf) {
            g++;
            g_f0 += g_nf;
            g_nf = g_base + (g < g_extra ? 1 : 0);
        }
        const size_t at = (size_t)g_f0 * dm.slots_per_frame + (size_t)slot * (size_t)g_nf + (size_t)(f - g_f0);
        f3 cur;
        if (sky_constant) {
            cur = sky_value;
            last = cur;
        } else if (slow) {   // rgba8 load of progressive_rendering.glsl:33
            const uint32_t q = s_val[wave][my_rank * (uint32_t)fp.n_frames + (uint32_t)f];
            cur = mk3(from_unorm8(q & 255u), from_unorm8((q >> 8) & 255u), from_unorm8((q >> 16) & 255u));
            last = cur;
        } else if (culled) {
            uint32_t sx, sy;
            const Ray ray = primary_ray(cam, fp.width, fp.height, px, py, fp.frame_index + (uint32_t)f, sx, sy);
            cur = mk3(0.0f, 0.0f, 0.0f) + mk3(1.0f, 1.0f, 1.0f) * JPT_SKY(ray.d);
            if (fp.accum_mode == 0) {  // rgba8 store of main.glsl:434, load of progressive_rendering.glsl:33
                last = mk3(from_unorm8(unorm8(cur.x)), from_unorm8(unorm8(cur.y)), from_unorm8(unorm8(cur.z)));
                cur = last;
            } else {
                last = cur;
            }
        } else if (fp.accum_mode == 0) {
            const uint32_t q = stream_ldu(&wb.fin8[at]);
            cur = mk3(from_unorm8(q & 255u), from_unorm8((q >> 8) & 255u), from_unorm8((q >> 16) & 255u));
            last = cur;   // (display_mode 1 shows the last frame's rgba8 image itself: quantising it again gives the same bytes)
        } else {
            const float4 r = stream_ld4(&wb.rad[at]);
            cur = mk3(r.x, r.y, r.z);
            last = cur;
        }
        sum = have_prev ? cur + sum : cur;  // progressive_rendering.glsl:34-36
        have_prev = true;
    }
    if (fp.n_frames > 0) {
        stream_st4(&accum[idx], make_float4(sum.x, sum.y, sum.z, 1.0f));
        const float fc = (float)(fp.frame_count + (uint32_t)fp.n_frames - 1u);
        const f3 col = fp.display_mode == 1 ? last : aces_film(mk3(sum.x / fc, sum.y / fc, sum.z / fc) * 1.0f);
        stream_stu(&ldr[idx], unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xFF000000u);
        if (depth_out) {
            const float dist = culled ? cam.far_ : wb.first_depth[slot];
            stream_stf(&depth_out[idx], cam.far_ / (cam.far_ - cam.near_) * (1.0f - cam.near_ / dist));  // main.glsl:432
        }
    }
}

#endif  // JPT_ENV < 2

#endif  // JPT_LENS, JPT_CAMERA_MODEL, JPT_BAKE, JPT_PROBE, JPT_CUBE

#undef JPT_ENV_NAME
#undef JPT_ENV_PARAM
#undef JPT_ENV_ARG
#undef JPT_NEE_PARAM
#undef JPT_NEE_ARG
#undef JPT_SKY
#ifdef JPT_PDF
#undef JPT_PDF
#endif
#ifdef JPT_LTOTAL
#undef JPT_LTOTAL
#undef JPT_MISS_WEIGHT
#undef JPT_HIT_WEIGHT
#endif
