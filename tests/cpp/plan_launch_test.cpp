// plan_launch_test.cpp -- every rule of jpt::plan_launch (csrc/jpt_render.cpp) against a fake PlanDevice, on host-only contexts whose
// fields are set directly: no device is touched, nothing is allocated.  One line per row of tests/test_plan_launch_host.py, which
// builds this program, runs it with JPT_PIPELINE, JPT_PIPE_SLOTS and JPT_GROUPS unset and compares the lines.
// Sizes are width x local_rows x frames; "native": JPT_TREE_NATIVE_REACH with an empty flattened scene; r is a default Wf2Render.
#include "../../gdpathtracing_amd/csrc/jpt_ctx.h"

#include <cstdio>

namespace {

// the fake device: what each question answers, how often it was asked, and the groups the last group_streams call named
struct Fake {
    bool six = false, idle = false, slot = true;
    int groups = 0;
    int n_six = 0, n_idle = 0, n_slot = 0, n_groups = 0, asked_groups = 0;
} g;
bool fake_six(jpt_ctx*) { g.n_six++; return g.six; }
bool fake_idle(jpt_ctx*) { g.n_idle++; return g.idle; }
bool fake_slot(jpt_ctx*, int) { g.n_slot++; return g.slot; }
int fake_groups(jpt_ctx*, int groups) { g.n_groups++; g.asked_groups = groups; return g.groups; }
const PlanDevice kFake{fake_six, fake_idle, fake_slot, fake_groups};

enum How { kBlocking, kCounted, kAsync };

jpt_ctx* context(int32_t w, int32_t rows, int32_t tree = JPT_TREE_NATIVE_REACH)
{
    jpt_ctx* c = nullptr;
    if (jpt_create(JPT_DEVICE_HOST_ONLY, &c) != JPT_OK || !c) {
        std::fprintf(stderr, "jpt_create failed\n");
        std::exit(2);
    }
    c->scene.tree = tree;
    c->width = w;
    c->height = c->local_rows = rows;
    c->max_bounces = 4;
    return c;
}

// one call of plan_launch, printed: the plan, the fake's call counts since the row began, and the plan's memory
void plan(const char* row, jpt_ctx* c, int32_t n_frames, How how)
{
    const FrameParams fp{c->width, c->height, c->local_rows, c->rank, c->world, c->max_bounces, c->accum_mode, 1u, c->frame_count + 1u, n_frames, -1, 0, c->debug_steps ? 1 : 0};
    const Wf2Render r{};
    const LaunchPlan p = plan_launch(c, fp, r, how == kCounted, how != kAsync, kFake);
    static const char* const route[] = {"kReference", "kStream", "kSlot"};
    std::printf("%s: %s slot %d slots %d groups %d chain %d | asked six %d idle %d slot_stream %d group_streams %d (for %d) | last_pipe_slots %d idle_streak %d\n",
                row, route[p.route], p.slot, p.slots, p.groups, p.chain, g.n_six, g.n_idle, g.n_slot, g.n_groups, g.asked_groups,
                c->pipe.last_pipe_slots, c->pipe.idle_streak);
}

// rows 9 to 14 start here: async, 64 x 64 x 1, six_queues false, idle false, slot_stream true, async_seq 5
jpt_ctx* queued_context()
{
    g = Fake();
    jpt_ctx* c = context(64, 64);
    c->pipe.async_seq = 5;
    return c;
}

}  // namespace

int main()
{
    jpt_ctx* c;
    // 1, 2: the reference-layout kernel and DEBUG_STEPS are planned before anything is asked
    g = Fake(); c = context(64, 64); c->kernel_variant = JPT_KERNEL_REFERENCE_LAYOUT; plan("1", c, 1, kAsync); jpt_destroy(c);
    g = Fake(); c = context(64, 64); c->debug_steps = true; plan("2", c, 1, kAsync); jpt_destroy(c);
    // 3, 4: a small blocking render; the plan's memory is a queued render's (7 and 2 are marks)
    g = Fake(); c = context(64, 64); c->pipe.last_pipe_slots = 7; c->pipe.idle_streak = 2; plan("3", c, 1, kBlocking); jpt_destroy(c);
    g = Fake(); c = context(64, 64, JPT_TREE_REFERENCE_EXACT); plan("4", c, 1, kBlocking); jpt_destroy(c);
    // 5 to 8: frame groups from 12 Mi paths, where the helper streams can be made, not for counted renders
    g = Fake(); g.groups = 1; c = context(1920, 1080); plan("5", c, 8, kBlocking); jpt_destroy(c);
    g = Fake(); g.groups = 0; c = context(1920, 1080); plan("6", c, 8, kBlocking); jpt_destroy(c);
    g = Fake(); g.groups = 1; c = context(1280, 720); plan("7", c, 4, kBlocking); jpt_destroy(c);
    g = Fake(); g.groups = 1; c = context(1920, 1080); plan("8", c, 8, kCounted); jpt_destroy(c);
    // 9 to 13: queued renders
    c = queued_context(); plan("9", c, 1, kAsync); jpt_destroy(c);
    c = queued_context(); g.six = true; plan("10", c, 1, kAsync); jpt_destroy(c);
    c = queued_context(); c->pipe.max_slots = 1; plan("11", c, 1, kAsync); jpt_destroy(c);
    c = queued_context(); c->kernel_timing = true; c->pipe.idle_streak = 2; plan("12", c, 1, kAsync); jpt_destroy(c);
    c = queued_context(); g.slot = false; plan("13", c, 1, kAsync); jpt_destroy(c);
    // 14: the lone-async fallback from the third idle render in a row, until a render finds work in flight
    c = queued_context();
    g.idle = true;
    plan("14a", c, 1, kAsync); plan("14b", c, 1, kAsync); plan("14c", c, 1, kAsync); plan("14d", c, 1, kAsync);
    g.idle = false;
    plan("14e", c, 1, kAsync);
    jpt_destroy(c);
    // 15: a workspace past 24 GiB -- the frame count is found by asking wf2_workspace_bytes
    c = queued_context();
    c->width = c->height = c->local_rows = 8192;
    int32_t frames = 1;
    while (frames < 4096 && wf2_workspace_bytes(c->width, c->local_rows, frames, c->max_bounces, Lighting()) <= ((size_t)24 << 30)) frames *= 2;
    std::printf("15 size: huge %d\n", wf2_workspace_bytes(c->width, c->local_rows, frames, c->max_bounces, Lighting()) > ((size_t)24 << 30) ? 1 : 0);
    plan("15", c, frames, kAsync);
    jpt_destroy(c);
    return 0;
}
