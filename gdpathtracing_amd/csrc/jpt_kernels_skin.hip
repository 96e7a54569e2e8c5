// jpt_kernels_skin.hip -- posing a committed mesh on the device (jpt_scene_pose_mesh): blend shapes and linear blend skinning of the
// rig kept on the device (jpt_scene_set_mesh_rig) into the vertex and normal arrays the mesh refit reads (MeshRefitArgs::verts /
// normals, jpt_kernels_mesh.hip).  The arithmetic is jpt_skin.h's; the host halves below check and pack a rig, for the context
// calls and for jpt_debug_skin alike.
#include <cmath>
#include <cstring>

#include "jpt_kernels.h"
#include "jpt_skin.h"

namespace jpt {

namespace {

// One thread per vertex of the mesh; the lanes gather their bones from the palette in global memory with 16-byte loads (it is a few KB
// that every block reads: the L2 holds it.  An LDS-staged palette was measured and did not pay: LAB_NOTEBOOK.md).  The host has
// checked that every bone index of the rig is below n_bones (jpt_scene_pose_mesh), so no gather leaves the palette.
template <int K>
__global__ __launch_bounds__(256) void mesh_skin_kernel(SkinArgs a)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.rig.n_vertices) return;
    f3 p, n;
    skin_vertex<K>(a.rig, v, a.active, a.n_active, a.palette, p, n);
    float* po = a.verts_out + (size_t)v * 3;
    po[0] = p.x; po[1] = p.y; po[2] = p.z;
    if (a.rig.bind_nrm) {
        float* no = a.normals_out + (size_t)v * 3;
        no[0] = n.x; no[1] = n.y; no[2] = n.z;
    }
}

size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

}  // namespace

void launch_mesh_skin(hipStream_t stream, const SkinArgs& a)
{
    if (a.rig.n_vertices == 0) return;
    const dim3 grid((a.rig.n_vertices + 255u) / 256u), block(256);
    if (a.influences == 8) hipLaunchKernelGGL(mesh_skin_kernel<8>, grid, block, 0, stream, a);
    else if (a.influences == 4) hipLaunchKernelGGL(mesh_skin_kernel<4>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(mesh_skin_kernel<0>, grid, block, 0, stream, a);
}

int check_skin_rig(const char* call, const SkinPiece* pieces, int32_t n_pieces, int32_t influences, int32_t n_shapes, bool with_normals,
                   SkinRigInfo& info, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    if (influences != 0 && influences != 4 && influences != 8) return why = who + "influences must be 0, 4 or 8", JPT_E_INVALID;
    if (n_shapes < 0) return why = who + "negative blend shape count", JPT_E_INVALID;
    if (n_shapes > kSkinMaxShapes) return why = who + "more than 256 blend shapes", JPT_E_LIMIT;
    if (influences == 0 && n_shapes == 0) return why = who + "a rig needs bones or blend shapes", JPT_E_INVALID;
    if (n_pieces < 0 || (n_pieces && !pieces)) return why = who + "bad rig array", JPT_E_INVALID;
    int with_vertices = 0, with_dn = 0;
    size_t nv = 0;
    for (int32_t l = 0; l < n_pieces; l++) {
        const SkinPiece& x = pieces[l];
        if (x.n_vertices <= 0) continue;
        with_vertices++;
        nv += (size_t)x.n_vertices;
        if (influences && (!x.bones || !x.weights)) return why = who + "a surface with vertices needs bones and weights", JPT_E_INVALID;
        if (n_shapes && !x.dpos) return why = who + "a surface with vertices needs position deltas", JPT_E_INVALID;
        with_dn += (n_shapes && x.dnrm) ? 1 : 0;
    }
    if (with_dn != 0 && with_dn != with_vertices) return why = who + "give normal deltas for every surface of the mesh or for none", JPT_E_INVALID;
    if (with_dn && !with_normals) return why = who + "normal deltas need bind normals", JPT_E_INVALID;
    int32_t max_bone = -1;
    for (int32_t l = 0; l < n_pieces; l++) {
        const SkinPiece& x = pieces[l];
        if (x.n_vertices <= 0) continue;
        const size_t nk = (size_t)x.n_vertices * (size_t)influences;
        for (size_t i = 0; i < nk; i++) {
            if (x.bones[i] < 0 || x.bones[i] > kSkinMaxBone) return why = who + "bone index outside 0 .. 4095", JPT_E_LIMIT;
            max_bone = x.bones[i] > max_bone ? x.bones[i] : max_bone;
        }
    }
    for (int32_t l = 0; l < n_pieces; l++) {
        const SkinPiece& x = pieces[l];
        if (x.n_vertices <= 0) continue;
        const size_t nk = (size_t)x.n_vertices * (size_t)influences, nd = (size_t)n_shapes * (size_t)x.n_vertices * 3;
        for (size_t i = 0; i < nk; i++)
            if (!std::isfinite(x.weights[i])) return why = who + "bone weight is not finite", JPT_E_INVALID;
        for (size_t i = 0; i < nd; i++)
            if (!std::isfinite(x.dpos[i]) || (with_dn && !std::isfinite(x.dnrm[i]))) return why = who + "blend shape delta is not finite", JPT_E_INVALID;
    }
    info.n_vertices = (uint32_t)nv;
    info.influences = influences;
    info.n_shapes = n_shapes;
    info.max_bone = max_bone;
    info.with_normals = with_normals;
    info.with_dnrm = with_dn != 0;
    const size_t v3 = align16(nv * 3 * sizeof(float));
    size_t off = 0;
    info.off_pos = off, off += v3;
    info.off_nrm = off, off += with_normals ? v3 : 0;
    info.off_bones = off, off += align16(nv * (size_t)influences * sizeof(uint16_t));
    info.off_weights = off, off += align16(nv * (size_t)influences * sizeof(float));
    info.off_dpos = off, off += align16((size_t)n_shapes * nv * 3 * sizeof(float));
    info.off_dnrm = off, off += info.with_dnrm ? align16((size_t)n_shapes * nv * 3 * sizeof(float)) : 0;
    info.bytes = off;
    return JPT_OK;
}

void pack_skin_rig(const SkinRigInfo& info, const SkinPiece* pieces, int32_t n_pieces, char* out)
{
    std::memset(out, 0, info.bytes);
    const size_t nv = info.n_vertices, K = (size_t)info.influences;
    float* pos = reinterpret_cast<float*>(out + info.off_pos);
    float* nrm = reinterpret_cast<float*>(out + info.off_nrm);
    uint16_t* bones = reinterpret_cast<uint16_t*>(out + info.off_bones);
    float* weights = reinterpret_cast<float*>(out + info.off_weights);
    float* dpos = reinterpret_cast<float*>(out + info.off_dpos);
    float* dnrm = reinterpret_cast<float*>(out + info.off_dnrm);
    size_t v0 = 0;
    for (int32_t l = 0; l < n_pieces; l++) {
        const SkinPiece& x = pieces[l];
        if (x.n_vertices <= 0) continue;
        const size_t n = (size_t)x.n_vertices;
        std::memcpy(pos + v0 * 3, x.positions, n * 3 * sizeof(float));
        if (info.with_normals) std::memcpy(nrm + v0 * 3, x.normals, n * 3 * sizeof(float));
        for (size_t i = 0; i < n * K; i++) bones[v0 * K + i] = (uint16_t)x.bones[i];
        if (K) std::memcpy(weights + v0 * K, x.weights, n * K * sizeof(float));
        // the surface's deltas are shape-major over ITS vertices; the mesh's are shape-major over all of them
        for (size_t s = 0; s < (size_t)info.n_shapes; s++) {
            std::memcpy(dpos + (s * nv + v0) * 3, x.dpos + s * n * 3, n * 3 * sizeof(float));
            if (info.with_dnrm) std::memcpy(dnrm + (s * nv + v0) * 3, x.dnrm + s * n * 3, n * 3 * sizeof(float));
        }
        v0 += n;
    }
}

SkinRig skin_rig_view(const SkinRigInfo& info, const char* base)
{
    SkinRig r;
    r.bind_pos = reinterpret_cast<const float*>(base + info.off_pos);
    r.bind_nrm = info.with_normals ? reinterpret_cast<const float*>(base + info.off_nrm) : nullptr;
    r.bones = info.influences ? reinterpret_cast<const uint16_t*>(base + info.off_bones) : nullptr;
    r.weights = info.influences ? reinterpret_cast<const float*>(base + info.off_weights) : nullptr;
    r.dpos = info.n_shapes ? reinterpret_cast<const float*>(base + info.off_dpos) : nullptr;
    r.dnrm = info.with_dnrm ? reinterpret_cast<const float*>(base + info.off_dnrm) : nullptr;
    r.n_vertices = info.n_vertices;
    return r;
}

int check_skin_pose(const char* call, const SkinRigInfo& info, const float* bone_transforms12, uint32_t n_bones, const float* blend_weights,
                    uint32_t n_blend_weights, std::vector<SkinShape>& active, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    if (info.influences) {
        if (!bone_transforms12) return why = who + "null bone transforms", JPT_E_INVALID;
        if ((int64_t)n_bones <= (int64_t)info.max_bone) return why = who + "the rig names bone " + std::to_string(info.max_bone) + ": give more bone transforms", JPT_E_INVALID;
    }
    if (n_blend_weights != (uint32_t)info.n_shapes) return why = who + "one blend weight per blend shape of the rig", JPT_E_INVALID;
    if (n_blend_weights && !blend_weights) return why = who + "null blend weights", JPT_E_INVALID;
    active.clear();
    for (uint32_t s = 0; s < n_blend_weights; s++) {
        if (!std::isfinite(blend_weights[s])) return why = who + "blend weight is not finite", JPT_E_INVALID;
        if (blend_weights[s] != 0.0f) active.push_back(SkinShape{s, blend_weights[s]});
    }
    return JPT_OK;
}

}  // namespace jpt
