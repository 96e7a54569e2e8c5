// jpt_guide_kernel.h -- the guide pass of jpt_denoise (jpt_kernels_denoise.hip), included twice inside its anonymous namespace:
//   as it is              guide_kernel<W4>: the un-jittered pinhole ray through the pixel centre (cam.position, raster_direction) --
//                         the same source, token for token, and so the same gfx950 code as before the camera models existed;
//   JPT_CAMERA_MODEL      guide_cam_kernel<W4> (jpt_set_camera_model): one more parameter, the model (CamModelDev, by value), and
//                         the model's pixel-centre ray (camera_raster_ray, jpt_camera.h); position_t.w is the distance from that
//                         ray's own origin.
// Shared by the preprocessor, like the miss models of jpt_wf2_paths.h.  No include guard.
#ifdef JPT_CAMERA_MODEL
#define JPT_GUIDE_NAME guide_cam_kernel
#define JPT_GUIDE_PARAM , CamModelDev cm
#else
#define JPT_GUIDE_NAME guide_kernel
#define JPT_GUIDE_PARAM
#endif

template <bool W4>
__global__ __launch_bounds__(kGuideBlock) void JPT_GUIDE_NAME(WideSceneDev sc, SceneShading sh, RefCamera cam, int width, int height,
                                                            float4* __restrict__ position_t, float4* __restrict__ normal,
                                                            float4* __restrict__ albedo JPT_GUIDE_PARAM)
{
    constexpr int kDepth = kStackLds + kStackSpill;
    __shared__ int32_t stack[kDepth * kGuideBlock];
    const int x = (int)blockIdx.x * 8 + ((int)threadIdx.x & 7), y = (int)blockIdx.y * 8 + ((int)threadIdx.x >> 3);
    if (x >= width || y >= height) return;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
#ifdef JPT_CAMERA_MODEL
    const Ray ray = camera_raster_ray(cam, cm, width, height, (float)x + 0.5f, (float)y + 0.5f);
    const f3 o = ray.o, d = ray.d;
#else
    const f3 o = mk3(cam.position.x, cam.position.y, cam.position.z);
    float ww;
    const f3 d = raster_direction(cam, width, height, (float)x + 0.5f, (float)y + 0.5f, ww);
#endif
    const typename Traversal<false, W4>::Stack st{&stack[threadIdx.x], nullptr, kGuideBlock, kDepth, 0};
    DevCounters cnt = {};
    Traversal<false, W4> tr;
    tr.begin(sc, o, d);
    while (tr.step(sc, st, cnt)) {
    }
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, -1.0f), gn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ga = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if (tr.hit.t < 1e9f) {
        Hit h;
        h.t = tr.hit.t;
        h.u = tr.hit.u;
        h.v = tr.hit.v;
        h.tri = tr.hit.tri;
        h.inst = (tr.hit.inst >> kInstBits) & kInstMask;   // the instance whose local ray found the triangle kept
        const RefInstance& b = sh.instances[h.inst];
        h.lo = xform_point(b.inverse_transform, o);
        h.ld = xform_dir(b.inverse_transform, d);
        const Shading s = get_shading_data<3>(sh, h, tr.hit.front, load_shade_tri(sh, h.tri));
        gp = make_float4(s.position.x, s.position.y, s.position.z, length3(s.position - o));
        gn = make_float4(s.normal.x, s.normal.y, s.normal.z, 0.0f);
        if (!(light_lum(s.emission.x, s.emission.y, s.emission.z) > 0.0f))   // (a light's face is not divided by its albedo)
            ga = make_float4(s.diffuse_albedo.x + s.fresnel_0.x, s.diffuse_albedo.y + s.fresnel_0.y, s.diffuse_albedo.z + s.fresnel_0.z, 0.0f);
    }
    position_t[idx] = gp;
    normal[idx] = gn;
    albedo[idx] = ga;
}

#undef JPT_GUIDE_NAME
#undef JPT_GUIDE_PARAM
