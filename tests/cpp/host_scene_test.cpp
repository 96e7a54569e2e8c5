// host_scene_test.cpp -- the scene on the host through the C ABI alone (include/jpt.h), on JPT_DEVICE_HOST_ONLY contexts: no device.
// begin, commit, set transform, update; upload (native and as given), an accepted jpt_scene_update_reference_tlas and a rejected one;
// share; destroy.  After every step it prints the step's return code and, for each reference buffer, its size and an FNV-1a checksum
// of its bytes.  tests/test_host_scene_cpp_host.py builds and runs this program and compares what it prints with a recording made
// before the host scene got a file of its own (tests/golden/host_scene_test.txt).  A step that fails where it should not ends the
// program with status 1.  Stand-alone (its own main), so that it can also be built with a sanitizer, together with the host objects.
#include "../../include/jpt.h"

#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

const char* kBufName[9] = {"tri_geometry", "tri_data", "materials", "bvh_nodes", "instances", "tlas_nodes", "triangles", "reach_triangles", "reach_instances"};

std::vector<unsigned char> buffer(jpt_ctx* c, int32_t which)
{
    size_t n = 0;
    if (jpt_scene_get_reference_buffer(c, which, nullptr, 0, &n) != JPT_OK) {
        std::fprintf(stderr, "jpt_scene_get_reference_buffer(%d): %s\n", which, jpt_last_error(c));
        std::exit(1);
    }
    std::vector<unsigned char> out(n);
    if (jpt_scene_get_reference_buffer(c, which, out.data(), out.size(), &n) != JPT_OK || n != out.size()) std::exit(1);
    return out;
}

void dump(const char* step, int rc, jpt_ctx* c)
{
    std::printf("%s: rc %d tree %d note \"%s\"\n", step, rc, jpt_scene_tree_kind(c), jpt_scene_upload_note(c));
    for (int32_t which = 0; which < 9; which++) {
        const std::vector<unsigned char> b = buffer(c, which);
        uint64_t h = 1469598103934665603ull;
        for (unsigned char x : b) h = (h ^ x) * 1099511628211ull;
        std::printf("  %-16s %8zu %016llx\n", kBufName[which], b.size(), (unsigned long long)h);
    }
}

void must(int rc, const char* what, jpt_ctx* c)
{
    if (rc == JPT_OK) return;
    std::fprintf(stderr, "%s: %d %s\n", what, rc, jpt_last_error(c));
    std::exit(1);
}

// a unit quad in the plane y = 0 (one surface) and a tent of two quads (two surfaces)
const float kQuadV[12] = {-1, 0, -1, 1, 0, -1, 1, 0, 1, -1, 0, 1};
const float kQuadN[12] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0};
const float kTentV[12] = {-1, 0, -1, 0, 1, -1, 0, 1, 1, -1, 0, 1};
const float kTentW[12] = {0, 1, -1, 1, 0, -1, 1, 0, 1, 0, 1, 1};
const float kQuadUV[8] = {0, 0, 1, 0, 1, 1, 0, 1};
const int32_t kQuadI[6] = {0, 1, 2, 0, 2, 3};

void add_scene(jpt_ctx* c)
{
    must(jpt_scene_begin(c), "jpt_scene_begin", c);
    const jpt_surface quad = {kQuadV, kQuadN, kQuadUV, kQuadI, 4, 6};
    const jpt_surface tent[2] = {{kTentV, kQuadN, kQuadUV, kQuadI, 4, 6}, {kTentW, kQuadN, kQuadUV, kQuadI, 4, 6}};
    uint32_t quad_id = 0, tent_id = 0;
    must(jpt_scene_add_mesh(c, &quad, 1, &quad_id), "jpt_scene_add_mesh", c);
    must(jpt_scene_add_mesh(c, tent, 2, &tent_id), "jpt_scene_add_mesh", c);
    const float floor12[12] = {4, 0, 0, 0, 1, 0, 0, 0, 4, 0, -1, 0};
    const float left12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -1.5f, -1, 0.25f};
    const float right12[12] = {0, 0, 1, 0, 1.5f, 0, -1, 0, 0, 1.5f, -1, -0.5f};
    const int32_t one[1] = {1}, two[2] = {2, 1};
    must(jpt_scene_add_instance(c, quad_id, floor12, one, 1), "jpt_scene_add_instance", c);
    must(jpt_scene_add_instance(c, tent_id, left12, two, 2), "jpt_scene_add_instance", c);
    must(jpt_scene_add_instance(c, tent_id, right12, two, 2), "jpt_scene_add_instance", c);
    float materials[3][16] = {};   // GpuMaterial, 64 B: albedo, emission, metallic, roughness, texture index, padding
    for (int m = 0; m < 3; m++) {
        materials[m][0] = 0.25f * (float)(m + 1), materials[m][1] = 0.5f, materials[m][2] = 0.75f, materials[m][3] = 1.0f;
        materials[m][7] = 1.0f, materials[m][9] = 1.0f;
        const int32_t no_texture = -1;
        std::memcpy(&materials[m][10], &no_texture, sizeof no_texture);
    }
    materials[2][4] = materials[2][5] = materials[2][6] = 1.0f, materials[2][7] = 5.0f;   // an emitter
    must(jpt_scene_set_materials(c, materials, 3), "jpt_scene_set_materials", c);
}

const float kMoved12[12] = {0.5f, 0, 0.5f, 0, 1, 0, -0.5f, 0, 0.5f, -2.0f, -0.5f, 1.0f};

jpt_ctx* create()
{
    jpt_ctx* c = nullptr;
    if (jpt_create(JPT_DEVICE_HOST_ONLY, &c) != JPT_OK || !c) {
        std::fprintf(stderr, "jpt_create: %s\n", jpt_last_error(nullptr));
        std::exit(1);
    }
    return c;
}

int upload(jpt_ctx* c, const std::vector<unsigned char> (&b)[6], int32_t mode)
{
    must(jpt_set_upload_mode(c, mode), "jpt_set_upload_mode", c);
    return jpt_scene_upload_reference_layout(c, b[0].data(), (uint32_t)(b[0].size() / 48), b[1].data(), b[2].data(), (uint32_t)(b[2].size() / 64), b[3].data(),
                                             (uint32_t)(b[3].size() / 48), b[4].data(), (uint32_t)(b[4].size() / 176), b[5].data(), (uint32_t)(b[5].size() / 32),
                                             nullptr, 0, 0);
}

}  // namespace

int main()
{
    // begin, commit, set transform, update -- with each builder
    const int32_t builders[3] = {JPT_BUILD_REFERENCE_EXACT, JPT_BUILD_SAH, JPT_BUILD_SAH_WATERTIGHT};
    const char* builder_name[3] = {"exact", "sah", "watertight"};
    jpt_ctx* committed[3];
    char step[96];
    for (int k = 0; k < 3; k++) {
        jpt_ctx* c = committed[k] = create();
        add_scene(c);
        std::snprintf(step, sizeof step, "commit %s", builder_name[k]);
        dump(step, jpt_scene_commit(c, builders[k]), c);
        must(jpt_scene_set_instance_transform(c, 1, kMoved12), "jpt_scene_set_instance_transform", c);
        std::snprintf(step, sizeof step, "set transform %s", builder_name[k]);
        dump(step, JPT_OK, c);   // (the arrays move at the update, not before)
        std::snprintf(step, sizeof step, "update %s", builder_name[k]);
        dump(step, jpt_scene_update_tlas(c), c);
    }
    // the arrays a host would upload: the reference-exact commit's, before and after the move
    jpt_ctx* fresh = create();
    add_scene(fresh);
    must(jpt_scene_commit(fresh, JPT_BUILD_REFERENCE_EXACT), "jpt_scene_commit", fresh);
    std::vector<unsigned char> before[6], after[6];
    for (int32_t which = 0; which < 6; which++) before[which] = buffer(fresh, which), after[which] = buffer(committed[0], which);
    std::vector<unsigned char> bad = after[5];
    if (bad.size() < 32) return 1;
    std::memset(bad.data() + 12, 0xff, 4);   // TLASNode::leftRight of slot 0, the root: both children out of range
    // upload, accepted update, rejected update -- native and as given
    const int32_t modes[2] = {JPT_UPLOAD_NATIVE_TREE, JPT_UPLOAD_WALK_AS_GIVEN};
    const char* mode_name[2] = {"native", "as given"};
    jpt_ctx* uploaded[2];
    for (int k = 0; k < 2; k++) {
        jpt_ctx* c = uploaded[k] = create();
        std::snprintf(step, sizeof step, "upload %s", mode_name[k]);
        dump(step, upload(c, before, modes[k]), c);
        std::snprintf(step, sizeof step, "accepted update %s", mode_name[k]);
        dump(step, jpt_scene_update_reference_tlas(c, after[4].data(), (uint32_t)(after[4].size() / 176), after[5].data(), (uint32_t)(after[5].size() / 32)), c);
        std::snprintf(step, sizeof step, "rejected update %s", mode_name[k]);
        const int rc = jpt_scene_update_reference_tlas(c, after[4].data(), (uint32_t)(after[4].size() / 176), bad.data(), (uint32_t)(bad.size() / 32));
        std::printf("  \"%s\"\n", jpt_last_error(c));
        dump(step, rc, c);
    }
    // share: from a commit whose transforms moved since its last update, and from an upload
    jpt_ctx* copy = create();
    must(jpt_scene_set_instance_transform(committed[1], 2, kMoved12), "jpt_scene_set_instance_transform", committed[1]);
    dump("share from sah", jpt_scene_share(copy, committed[1]), copy);
    dump("the source after it", JPT_OK, committed[1]);
    must(jpt_scene_set_instance_transform(copy, 0, kMoved12), "jpt_scene_set_instance_transform", copy);
    dump("update of the copy", jpt_scene_update_tlas(copy), copy);
    dump("share from native upload", jpt_scene_share(copy, uploaded[0]), copy);
    // destroy
    jpt_destroy(copy);
    jpt_destroy(fresh);
    for (jpt_ctx* c : committed) jpt_destroy(c);
    for (jpt_ctx* c : uploaded) jpt_destroy(c);
    jpt_destroy(nullptr);
    std::printf("destroyed\n");
    return 0;
}
