"""The refusals the post stages open with -- the calls that read the progressive sum on the context's stream: jpt_denoise, jpt_bake_finish,
jpt_bake_finish_directional, jpt_display, jpt_meter, jpt_noise_estimate, jpt_probe_project, jpt_reflection_prefilter and jpt_encode's mean
source -- on a host-only context: the denoising mode, DEBUG_STEPS and the partition are asked before the device in eight of the nine, so each is
reached without one.  Return code and the whole jpt_last_error text against a literal table, written down from the library as it was before the
refusals were gathered into one helper (csrc/jpt_post.cpp)."""
import pytest

from gdpathtracing_amd import capi, host

E_DEVICE, E_STATE = -2, -4   # JPT_E_DEVICE, JPT_E_STATE of include/jpt.h

MODE = ": the denoising mode must be JPT_DENOISE_PROGRESSIVE"
STEPS = ": the accumulation holds DEBUG_STEPS counts, not radiance (jpt_set_debug_steps)"
WORLD = " needs the whole image on one context (world == 1)"

# call -> (how it is made, the text under: another denoising mode, DEBUG_STEPS, world == 2, none of them)
TABLE = {
    "jpt_denoise": (lambda L, h: L.jpt_denoise(h),
                    "jpt_denoise filters the progressive accumulation" + MODE,
                    "jpt_denoise" + STEPS,
                    "jpt_denoise" + WORLD,
                    "host-only context: jpt_denoise runs on the device"),
    "jpt_bake_finish": (lambda L, h: L.jpt_bake_finish(h),
                        "jpt_bake_finish filters the progressive accumulation" + MODE,
                        "jpt_bake_finish" + STEPS,
                        "jpt_bake_finish" + WORLD,
                        "jpt_bake_finish: host-only context: it runs on the device"),
    "jpt_bake_finish_directional": (lambda L, h: L.jpt_bake_finish_directional(h),
                                    "jpt_bake_finish_directional filters the progressive moments" + MODE,
                                    "jpt_bake_finish_directional: DEBUG_STEPS renders make no moments (jpt_set_debug_steps)",
                                    "jpt_bake_finish_directional" + WORLD,
                                    "jpt_bake_finish_directional: host-only context: it runs on the device"),
    "jpt_display": (lambda L, h: L.jpt_display(h),
                    "jpt_display grades the progressive accumulation" + MODE,
                    "jpt_display" + STEPS,
                    "jpt_display" + WORLD + ": the bloom reads rows a partition does not hold",
                    "host-only context: jpt_display runs on the device"),
    "jpt_meter": (lambda L, h: L.jpt_meter(h),
                  "jpt_meter meters the progressive accumulation" + MODE,
                  "jpt_meter" + STEPS,
                  "jpt_meter" + WORLD,
                  "host-only context: jpt_meter runs on the device"),
    "jpt_noise_estimate": (lambda L, h: L.jpt_noise_estimate(h),
                           "jpt_noise_estimate reads the progressive accumulation" + MODE,
                           "jpt_noise_estimate" + STEPS,
                           "jpt_noise_estimate" + WORLD,
                           "host-only context: jpt_noise_estimate runs on the device"),
    "jpt_probe_project": (lambda L, h: L.jpt_probe_project(h, capi.PROBE_RADIANCE),
                          "jpt_probe_project projects the progressive accumulation" + MODE,
                          "jpt_probe_project" + STEPS,
                          "jpt_probe_project" + WORLD + ": the gathering context projects",
                          "jpt_probe_project: host-only context: it runs on the device"),
    "jpt_reflection_prefilter": (lambda L, h: L.jpt_reflection_prefilter(h),
                                 "jpt_reflection_prefilter filters the progressive accumulation" + MODE,
                                 "jpt_reflection_prefilter" + STEPS,
                                 "jpt_reflection_prefilter" + WORLD + ": the gathering context filters",
                                 "jpt_reflection_prefilter: host-only context: it runs on the device"),
}
# jpt_encode asks for the device first: on a host-only context that is its answer whatever else is set
ENCODE_HOST_ONLY = "jpt_encode: host-only context: it runs on the device"

# condition -> (set it, put it back), in the order the calls ask
CONDITIONS = (
    (lambda L, h: L.jpt_set_denoising_mode(h, capi.DENOISE_TEMPORAL), lambda L, h: L.jpt_set_denoising_mode(h, capi.DENOISE_PROGRESSIVE)),
    (lambda L, h: L.jpt_set_debug_steps(h, 1), lambda L, h: L.jpt_set_debug_steps(h, 0)),
    (lambda L, h: L.jpt_set_partition(h, 0, 2), lambda L, h: L.jpt_set_partition(h, 0, 1)),
)


@pytest.fixture()
def ctx():
    c = host.Context(-1)
    yield c
    c.close()


def refusal(L, h, call):
    L.jpt_set_kernel_timing(h, 0)   # (a call that succeeds and leaves the error text alone: the text below is this call's)
    rc = call(L, h)
    return rc, L.jpt_last_error(h).decode()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_refusals_in_their_order(ctx, name):
    L = capi.lib()
    call, mode, steps, world, host_only = TABLE[name]
    for (on, off), want in zip(CONDITIONS, (mode, steps, world)):
        assert on(L, ctx.h) == capi.OK
        assert refusal(L, ctx.h, call) == (E_STATE, want)
        assert off(L, ctx.h) == capi.OK
    assert refusal(L, ctx.h, call) == (E_DEVICE, host_only)
    # the order: with all three set the mode is named, without the mode DEBUG_STEPS, without both the partition
    for on, _ in CONDITIONS:
        assert on(L, ctx.h) == capi.OK
    for (_, off), want in zip(CONDITIONS, (mode, steps, world)):
        assert refusal(L, ctx.h, call) == (E_STATE, want)
        assert off(L, ctx.h) == capi.OK
    assert refusal(L, ctx.h, call) == (E_DEVICE, host_only)


def test_jpt_encode_asks_for_the_device_first(ctx):
    L = capi.lib()
    call = lambda L, h: L.jpt_encode(h, capi.ENCODE_SOURCE_MEAN, 0, capi.ENCODE_RGBA16F)
    assert refusal(L, ctx.h, call) == (E_DEVICE, ENCODE_HOST_ONLY)
    for on, off in CONDITIONS:
        assert on(L, ctx.h) == capi.OK
        assert refusal(L, ctx.h, call) == (E_DEVICE, ENCODE_HOST_ONLY)
        assert off(L, ctx.h) == capi.OK
