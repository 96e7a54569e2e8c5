// jpt_tlas_rebuild.h -- the arithmetic of jpt_scene_rebuild_tlas, written once for the device (jpt_kernels_tlas.hip), for the host's
// mirror of it (the sky cull's boxes, jpt_scene_update.cpp) and for jpt_debug_tlas_order's host form: the sort key of an instance from its
// world box, and the fixed four-way topology over the sorted instances.  Every float step is one binary32 operation, a
// compare-and-select or a floor, in source order, compiled without contraction on both sides, so the two give the same bits.
#pragma once

#include "jpt_mesh_math.h"   // JPT_HD, ordered_key
#include "jpt_types.h"

#include <algorithm>
#include <vector>

namespace jpt {

constexpr uint32_t kTlasRebuildMaxInstances = 32767u;   // the instance index takes the key's low 15 bits
constexpr uint32_t kTlasLdsKeys = 2048u;   // up to here the sort's two key buffers are in LDS (2 x 16 KiB of the block's 49 KiB), beyond in device memory
constexpr int32_t kTlasKeyBoundsMin = 0x7f7fffff;           // ordered_key(+FLT_MAX) and ordered_key(-FLT_MAX): where the minimum and
constexpr int32_t kTlasKeyBoundsMax = (int32_t)0x80800000u;  // the maximum of the finite centres start (as the mesh bounds do)

// neither an infinity nor a NaN, by the exponent field
JPT_HD bool tlas_finite(float f)
{
    union {
        float f;
        uint32_t u;
    } v;
    v.f = f;
    return (v.u & 0x7f800000u) != 0x7f800000u;
}

JPT_HD float tlas_centre(float lo, float hi) { return (lo + hi) * 0.5f; }

// cells per unit along an axis whose finite centres span bmin .. bmax; 0 for an axis with no extent (or no finite centre)
JPT_HD float tlas_inv_extent(float bmin, float bmax)
{
    const float ext = bmax - bmin;
    return ext > 0.0f ? 1024.0f / ext : 0.0f;
}

// the centre's cell of 1024 along its axis: min(1023, floor((c - bmin) * inv)); a non-finite centre, and a product that is
// not a number (an extent beyond FLT_MAX), fall into cell 0 by compare-and-select, before any conversion
JPT_HD uint32_t tlas_cell(float c, float bmin, float inv)
{
    const float f = __builtin_floorf((c - bmin) * inv);
    const uint32_t q = f >= 1024.0f ? 1023u : (f >= 0.0f ? (uint32_t)f : 0u);
    return tlas_finite(c) ? q : 0u;
}

// bit i of a 10-bit number -> bit 3 i
JPT_HD uint32_t tlas_spread3(uint32_t v)
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Morton code, x in the highest bit of each triple, above the instance's index: unique per instance, 45 bits
JPT_HD uint64_t tlas_key(const float* lo, const float* hi, const float* bmin, const float* inv, uint32_t instance)
{
    const uint32_t qx = tlas_cell(tlas_centre(lo[0], hi[0]), bmin[0], inv[0]);
    const uint32_t qy = tlas_cell(tlas_centre(lo[1], hi[1]), bmin[1], inv[1]);
    const uint32_t qz = tlas_cell(tlas_centre(lo[2], hi[2]), bmin[2], inv[2]);
    const uint32_t code = (tlas_spread3(qx) << 2) | (tlas_spread3(qy) << 1) | tlas_spread3(qz);
    return ((uint64_t)code << 15) | (uint64_t)instance;
}

// ---- host only ----

// The host form of the order kernel: boxes at lo / hi (`stride` floats from one instance's to the next's), keys per instance (may be
// null) and the instance at each sorted position.
inline void tlas_order_host(const float* lo, const float* hi, size_t stride, uint32_t n, uint64_t* keys_out, uint32_t* sorted_out)
{
    int32_t kmin[3] = {kTlasKeyBoundsMin, kTlasKeyBoundsMin, kTlasKeyBoundsMin}, kmax[3] = {kTlasKeyBoundsMax, kTlasKeyBoundsMax, kTlasKeyBoundsMax};
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const float c = tlas_centre(lo[i * stride + k], hi[i * stride + k]);
            if (!tlas_finite(c)) continue;
            kmin[k] = std::min(kmin[k], ordered_key(c));
            kmax[k] = std::max(kmax[k], ordered_key(c));
        }
    float bmin[3], inv[3];
    for (int k = 0; k < 3; k++) {
        bmin[k] = from_ordered_key(kmin[k]);
        inv[k] = tlas_inv_extent(bmin[k], from_ordered_key(kmax[k]));
    }
    std::vector<uint64_t> keys(n);
    for (uint32_t i = 0; i < n; i++) keys[i] = tlas_key(lo + i * stride, hi + i * stride, bmin, inv, i);
    if (keys_out) std::copy(keys.begin(), keys.end(), keys_out);
    std::sort(keys.begin(), keys.end());
    for (uint32_t p = 0; p < n; p++) sorted_out[p] = (uint32_t)(keys[p] & 0x7fffu);
}

// The topology over n >= 2 sorted positions, a pure function of n: records numbered breadth first, record 0 the root over [0, n).
// A record over m <= 4 positions holds them as its first m slots; a record over more cuts its range into four consecutive parts of
// floor(m / 4) positions, one more for the first m mod 4: a part of one position is a leaf slot, a larger one a record of the next
// level, appended in slot order.  Slots: >= 0 a record, ~position a leaf, kEmptyChild.  At most ceil(log4 n) levels, and every
// record has two children or more, so there are at most n - 1.
struct TlasTemplate {
    uint32_t n = 0;
    std::vector<int32_t> child;   // 4 per record
    uint32_t n_records = 0, n_levels = 0;
};
inline void make_tlas_template(uint32_t n, TlasTemplate& t)
{
    t.n = n;
    t.child.clear();
    t.n_records = t.n_levels = 0;
    if (n < 2) return;
    struct Range {
        uint32_t first, count;
    };
    std::vector<Range> level{{0u, n}}, next;
    uint32_t numbered = 1;   // records numbered so far, this level's included
    while (!level.empty()) {
        next.clear();
        for (const Range& r : level) {
            int32_t slot[4] = {kEmptyChild, kEmptyChild, kEmptyChild, kEmptyChild};
            if (r.count <= 4) {
                for (uint32_t k = 0; k < r.count; k++) slot[k] = ~(int32_t)(r.first + k);
            } else {
                uint32_t first = r.first;
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t part = r.count / 4 + (k < r.count % 4 ? 1u : 0u);
                    if (part == 1) slot[k] = ~(int32_t)first;
                    else {
                        slot[k] = (int32_t)(numbered + next.size());
                        next.push_back({first, part});
                    }
                    first += part;
                }
            }
            t.child.insert(t.child.end(), slot, slot + 4);
        }
        numbered += (uint32_t)next.size();
        t.n_levels++;
        level.swap(next);
    }
    t.n_records = (uint32_t)(t.child.size() / 4);
}

// the template as records: a leaf slot over sorted position p names instance sorted[p]; boxes empty until a refit fills them
inline void tlas_template_records(const TlasTemplate& t, const uint32_t* sorted, std::vector<WideNode4>& out)
{
    out.assign(t.n_records, WideNode4{});
    for (uint32_t r = 0; r < t.n_records; r++)
        for (int k = 0; k < 4; k++) {
            const int32_t c = t.child[(size_t)r * 4 + k];
            WideNode4& o = out[r];
            o.child[k] = (c >= 0 || c == kEmptyChild) ? c : ~(int32_t)sorted[(uint32_t)~c];
            o.lo_x[k] = o.lo_y[k] = o.lo_z[k] = 3.402823466e38f;
            o.hi_x[k] = o.hi_y[k] = o.hi_z[k] = -3.402823466e38f;
        }
}

}  // namespace jpt
