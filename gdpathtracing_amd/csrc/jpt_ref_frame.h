// jpt_ref_frame.h -- ref_frame_kernel, the audit route's one kernel (jpt_kernels_ref.hip), which sees the paths' misses.  Included
// five times by jpt_kernels_ref.hip, as jpt_wf2_paths.h is by jpt_kernels_wf2.hip; launch_ref_frame switches on Lighting::kind:
//   JPT_ENV 0   ref_frame_kernel, main.glsl's gradient (sample_sky): the same source, token for token, as before the map existed;
//   JPT_ENV 1   ref_frame_kernel_env (jpt_set_environment): one more parameter, the map, and env_radiance at the miss;
//   JPT_ENV 2   ref_frame_kernel_mis (JPT_ENV_SAMPLING_MIS): also the map's sampling tables; below the last bounce each vertex casts
//               its map sample's shadow ray at once (ray_trace_tlas on the reference layout: a hit there is "blocked"), and a
//               miss at bounce >= 1 is weighted against that strategy -- the arithmetic of jpt_wf2_paths.h's *_mis kernels;
//   JPT_ENV 3   ref_frame_kernel_lt (JPT_LIGHT_SAMPLING_MIS): the emitter tables and the miss model as a run-time value (env_mode
//               0 gradient, 1 map, 2 map with JPT_ENV_SAMPLING_MIS); each vertex below the last bounce casts the map's shadow ray
//               (env_mode 2), then the emitters' (ray_trace_tlas with hitInfo.t preset to tmax: blocked when it ends below
//               tmax), and emission found at bounce >= 1 is weighted -- the arithmetic of jpt_wf2_paths.h's *_lt kernels.
//   JPT_ENV 4   ref_frame_kernel_tx (JPT_MATERIAL_EXT_TRANSMISSION over a scene with a transmissive material): ref_frame_kernel_lt with
//               emitter sampling on or off at run time (lt.n == 0) and the transmission lobe at every hit (transmission_step) --
//               the arithmetic of jpt_wf2_paths.h's *_tx kernels.
// (No include guard: that is the point.)
#if JPT_ENV >= 3
#if JPT_ENV == 4
#define JPT_ENV_NAME(name) name##_tx
#define JPT_LTOTAL (lt.n != 0u ? lt.marg[lt.n_blocks] : 0.0f)
#define JPT_MISS_WEIGHT env_miss_weight_tx
#define JPT_HIT_WEIGHT light_hit_weight_tx
#else
#define JPT_ENV_NAME(name) name##_lt
#define JPT_LTOTAL lt.marg[lt.n_blocks]
#define JPT_MISS_WEIGHT env_miss_weight
#define JPT_HIT_WEIGHT light_hit_weight
#endif
#define JPT_ENV_PARAM , EnvDev env, EnvSampDev es, LightDev lt, int env_mode
#define JPT_SKY(d) (env_mode != 0 ? env_radiance(env, d) : sample_sky(d))
#elif JPT_ENV == 2
#define JPT_ENV_NAME(name) name##_mis
#define JPT_ENV_PARAM , EnvDev env, EnvSampDev es
#define JPT_SKY(d) env_radiance(env, d)
#elif JPT_ENV
#define JPT_ENV_NAME(name) name##_env
#define JPT_ENV_PARAM , EnvDev env
#define JPT_SKY(d) env_radiance(env, d)
#else
#define JPT_ENV_NAME(name) name
#define JPT_ENV_PARAM
#define JPT_SKY(d) sample_sky(d)
#endif

// One dispatch of main.glsl (main.glsl:404-436) fused with one dispatch of progressive_rendering.glsl
// (:28-46) for the pixels of this context's partition.
template <bool COUNT, bool TIES>
__global__ __launch_bounds__(256, 5) void JPT_ENV_NAME(ref_frame_kernel)(RefSceneDev sc, TieShadowDev shadow, SceneShading sh, FrameParams fp, RefCamera cam,
                                                        float4* __restrict__ accum, uint32_t* __restrict__ ldr,
                                                        float* __restrict__ depth_out, DevCounters* __restrict__ counters, LensDev lens, CamModelDev cm, BakeDev bake, ProbeDev probe, CubeDev cube JPT_ENV_PARAM)
{
    // 8x32 pixel tiles: a wave covers 8x8 pixels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = blockIdx.x * 32 + wave * 8 + (lane & 7);
    const int ly = blockIdx.y * 8 + (lane >> 3);  // local row
    DevCounters cnt = {};
    if (px < fp.width && ly < fp.local_rows) {
        const int py = local_to_global_row(ly, fp);
        uint32_t sx, sy;
        Ray ray = primary_ray(cam, fp.width, fp.height, px, py, fp.frame_index, sx, sy);
        if (lens.radius > 0.0f) lens_ray(lens, sx, sy, ray);   // (jpt_set_lens; the host passes radius 0 with DEBUG_STEPS)
        if (cm.model != kCamPinhole) ray = camera_ray(cam, cm, fp.width, fp.height, px, py, fp.frame_index, sx, sy);   // (jpt_set_camera_model; likewise)
        bool lit = true;   // (jpt_set_bake_texels: an invalid texel traces nothing -- radiance 0, depth far; null images: a camera render,
                           // which the host also passes with DEBUG_STEPS)
        if (bake.normal != nullptr) {
            const size_t texel = (size_t)py * (size_t)fp.width + (size_t)px;
            const float4 bake_n = bake.normal[texel];
            lit = bake_texel_valid(bake_n);
            if (lit) ray = bake_ray(bake.position[texel], bake_n, px, py, fp.frame_index, sx, sy);
        }
        if (probe.position != nullptr) {   // (jpt_set_probes: a tile without a probe traces nothing, likewise; null: no probe render)
            uint32_t q, ci, cj;
            lit = probe_cell(probe, px, py, q, ci, cj);
            if (lit) ray = probe_ray(probe_position(probe, q), ci, cj, probe.tile_w(), probe.tile_h(), px, py, fp.frame_index, sx, sy);
        }
        if (cube.position != nullptr) {   // (jpt_set_reflection_probes: a strip without a probe traces nothing, likewise; null: no cube render)
            uint32_t q, cf, ci, cj;
            lit = cube_cell(cube, px, py, q, cf, ci, cj);
            if (lit) ray = cube_ray(cube_position(cube, q), cf, ci, cj, cube.face_size(), px, py, fp.frame_index, sx, sy);
        }
        float depth = cam.far_;
        f3 radiance = mk3(0.0f, 0.0f, 0.0f);
        f3 throughput = mk3(1.0f, 1.0f, 1.0f);
#if JPT_ENV >= 2
        float p_brdf = 0.0f;   // the BRDF density of the current ray's direction (bounces >= 1)
#endif
#if JPT_ENV >= 3
        const float ltotal = JPT_LTOTAL;
#endif
        if (fp.debug_steps) {   // #ifdef DEBUG_STEPS (main.glsl:358-361, 423-427): the primary ray's triangle tests / 256, depth = far
            RefHit hit;
            if (COUNT) cnt.rays++;
            (void)ray_trace_tlas<COUNT>(sc, ray, hit, cnt);
            const float g = clamp_((float)hit.steps / 256.0f, 0.0f, 1.0f);
            radiance = mk3(g, g, g);
        } else
        for (int i = 0; lit && i < fp.max_bounces + 1; i++) {  // main.glsl:377
            RefHit hit;
            if (COUNT) cnt.rays++;
            const bool is_hit = ray_trace_tlas<COUNT>(sc, ray, hit, cnt);
            if (!is_hit) {
#if JPT_ENV == 2
                if (i > 0) radiance = radiance + (throughput * JPT_SKY(ray.d)) * env_miss_weight(env, es, ray.d, p_brdf);
                else
#elif JPT_ENV >= 3
                if (i > 0 && env_mode == 2) radiance = radiance + (throughput * JPT_SKY(ray.d)) * JPT_MISS_WEIGHT(env, es, ray.d, p_brdf);
                else
#endif
                radiance = radiance + throughput * JPT_SKY(ray.d);
                break;
            }
            if (TIES && hit.tied) {
                // an exact distance tie: decided where the reference decides it (jpt_tie_walk.h) -- the leaves that hold
                // the tying triangles from one more walk with hitInfo.t preset, then the reference's own walk through
                // their ancestors (event counters: not those of a reference tree anyway)
                TieLeaves tl;
                RefHit again;
                DevCounters none = {};
                (void)ray_trace_tlas<false>(sc, ray, again, none, &shadow, &tl, hit.t);
                TraceHit xh;
                if (tl.n > 0 && tie_walk(shadow, sh.instances, shadow.tlas_current, tl, ray.o, ray.d, xh) && xh.t == hit.t) {
                    const uint32_t found_in = (xh.inst >> kInstBits) & kInstMask;
                    hit.u = xh.u;
                    hit.v = xh.v;
                    hit.tri = shadow.tri_native[xh.tri];
                    hit.front = xh.front;
                    hit.inst = xh.inst & kInstMask;
                    const RefInstance& fb = sc.instances[found_in];
                    hit.lo = xform_point(fb.inverse_transform, ray.o);
                    hit.ld = xform_dir(fb.inverse_transform, ray.d);
                }
            }
            if (COUNT) cnt.shaded_hits++;
            Hit h;
            h.t = hit.t; h.u = hit.u; h.v = hit.v; h.tri = hit.tri; h.inst = hit.inst; h.lo = hit.lo; h.ld = hit.ld;
            const Shading s = get_shading_data(sh, h, hit.front, load_shade_tri(sh, h.tri));
#if JPT_ENV >= 3
            if (i > 0) radiance = radiance + (throughput * s.emission) * JPT_HIT_WEIGHT(lt, ltotal, sh, h, s, ray.o, ray.d, &p_brdf);
            else
#endif
            radiance = radiance + throughput * s.emission;
            if (i == 0) depth = length3(s.position - ray.o);
#if JPT_ENV == 4
            // (the transmission lobe: a dielectric vertex casts no shadow ray, never ends the path and leaves the sentinel density)
            if (transmission_step(s, material_ext(sh, h, load_shade_tri(sh, h.tri)), hit.front, sx, sy, ray, throughput)) {
                p_brdf = kDeltaDensity;
                continue;
            }
#endif
#if JPT_ENV >= 2
            if (i < fp.max_bounces) {
                f3 l, c;
#if JPT_ENV >= 3
                if (env_mode == 2 && env_nee(s, env, es, sx, sy, throughput, l, c)) {
#else
                if (env_nee(s, env, es, sx, sy, throughput, l, c)) {
#endif
                    Ray sray;
                    sray.o = s.position + s.normal * 0.001f;
                    sray.d = l;
                    sray.rD = rcp3(l);
                    RefHit sh_hit;
                    DevCounters none = {};
                    if (!ray_trace_tlas<false>(sc, sray, sh_hit, none)) radiance = radiance + c;
                }
#if JPT_ENV >= 3
                f3 lo3, ll, lc;
                float tmax;
                if (ltotal > 0.0f && light_nee(s, lt, ltotal, sx, sy, throughput, lo3, ll, tmax, lc)) {
                    Ray sray;
                    sray.o = lo3;
                    sray.d = ll;
                    sray.rD = rcp3(ll);
                    RefHit sh_hit;
                    DevCounters none = {};
                    (void)ray_trace_tlas<false>(sc, sray, sh_hit, none, nullptr, nullptr, tmax);
                    if (!(sh_hit.t < tmax)) radiance = radiance + lc;
                }
#endif
            }
            if (!bounce_step_pdf(s, sx, sy, ray, throughput, p_brdf)) break;
#else
            if (!bounce_step(s, sx, sy, ray, throughput)) break;
#endif
        }
        depth = cam.far_ / (cam.far_ - cam.near_) * (1.0f - cam.near_ / depth);
        const size_t idx = (size_t)ly * fp.width + px;
        accumulate_pixel(fp, idx, radiance, accum, ldr);
        if (depth_out) depth_out[idx] = depth;
    }
    if (COUNT) flush_counters(cnt, counters);
}

#undef JPT_ENV_NAME
#undef JPT_ENV_PARAM
#undef JPT_SKY
#ifdef JPT_LTOTAL
#undef JPT_LTOTAL
#undef JPT_MISS_WEIGHT
#undef JPT_HIT_WEIGHT
#endif
