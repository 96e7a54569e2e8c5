"""jpt_scene_update_mesh / jpt_multi_update_mesh (deforming a committed mesh on the device): the argument and state checks run on
the host before any device work, so they are tested here on host-only contexts; the Python and C++ wrappers reach the calls."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # JPT_E_* (include/jpt.h)


def _small_scene():
    sc = scenes.demo_scene(n_tris=512)
    return sc


def _committed(builder):
    ctx = host.Context(-1)
    sc = _small_scene()
    ctx.build_scene(sc, builder)
    return ctx, sc


def _update_rc(ctx, mesh_id, mesh, n_surfaces=None):
    arr = host._update_surfaces(mesh)
    n = len(mesh.surfaces) if n_surfaces is None else n_surfaces
    rc = ctx._lib.jpt_scene_update_mesh(ctx.h, mesh_id, arr, n)
    msg = ctx._lib.jpt_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


def _deformed(mesh):
    m = copy.deepcopy(mesh)
    for s in m.surfaces:
        s.vertices = (s.vertices * np.float32(1.1)).astype(np.float32)
    return m


@pytest.mark.parametrize("builder,why", [(capi.BUILD_REFERENCE_EXACT, "JPT_BUILD_REFERENCE_EXACT"), (capi.BUILD_SAH, "reach records")])
def test_other_builders_are_refused_with_the_reason(hiplib, builder, why):
    ctx, sc = _committed(builder)
    rc, msg = _update_rc(ctx, 2, _deformed(sc.meshes[2]))
    assert rc == E_STATE
    assert why in msg and "JPT_BUILD_SAH_WATERTIGHT" in msg
    ctx.close()


def test_uploads_and_uncommitted_contexts_are_refused(hiplib):
    ctx = host.Context(-1)
    sc = _small_scene()
    rc, msg = _update_rc(ctx, 0, sc.meshes[0])
    assert rc == E_STATE and "jpt_scene_commit" in msg
    ctx.close()


def test_topology_changes_are_refused(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    blob = sc.meshes[2]
    # another index array (same length)
    m = copy.deepcopy(blob)
    m.surfaces[0].indices = m.surfaces[0].indices.copy()
    m.surfaces[0].indices[[0, 1]] = m.surfaces[0].indices[[1, 0]]
    rc, msg = _update_rc(ctx, 2, m)
    assert rc == E_INVALID and "topology changed: commit the scene again" in msg
    # another vertex count
    m = copy.deepcopy(blob)
    m.surfaces[0].vertices = np.concatenate([m.surfaces[0].vertices, m.surfaces[0].vertices[:1]])
    m.surfaces[0].normals = np.concatenate([m.surfaces[0].normals, m.surfaces[0].normals[:1]])
    rc, msg = _update_rc(ctx, 2, m)
    assert rc == E_INVALID and "topology changed" in msg
    # another surface count (the cube mesh has one surface per face group)
    cube = sc.meshes[1]
    rc, msg = _update_rc(ctx, 1, cube, n_surfaces=len(cube.surfaces) - 1)
    assert rc == E_INVALID and "topology changed" in msg
    # another index count
    m = copy.deepcopy(blob)
    m.surfaces[0].indices = m.surfaces[0].indices[:-3].copy()
    rc, msg = _update_rc(ctx, 2, m)
    assert rc == E_INVALID and "topology changed" in msg
    # a mesh's arrays given for another mesh
    rc, msg = _update_rc(ctx, 0, blob)
    assert rc == E_INVALID and "topology changed" in msg
    ctx.close()


def test_bad_mesh_id_and_arguments(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    rc, msg = _update_rc(ctx, len(sc.meshes), sc.meshes[2])
    assert rc == E_INVALID and "no such mesh" in msg
    rc = ctx._lib.jpt_scene_update_mesh(ctx.h, 2, None, 1)
    assert rc == E_INVALID
    # normals for some surfaces only
    cube = sc.meshes[1]
    arr = host._update_surfaces(cube)
    arr[0].normals = None
    rc = ctx._lib.jpt_scene_update_mesh(ctx.h, 1, arr, len(cube.surfaces))
    assert rc == E_INVALID and b"normals" in ctx._lib.jpt_last_error(ctx.h)
    ctx.close()


def test_a_valid_update_needs_the_device(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    for with_normals in (True, False):
        m = _deformed(sc.meshes[2])   # (kept alive: the surface array points into it)
        arr = host._update_surfaces(m, with_normals)
        rc = ctx._lib.jpt_scene_update_mesh(ctx.h, 2, arr, 1)
        assert rc == E_DEVICE and b"host-only" in ctx._lib.jpt_last_error(ctx.h)
    # the same vertices as committed are a valid update too; the host's copy of the scene stays usable (nothing ran)
    rc, msg = _update_rc(ctx, 2, sc.meshes[2])
    assert rc == E_DEVICE
    assert len(ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, np.dtype((np.uint8, 48)))) > 0
    ctx.update_tlas()
    info = (C.c_int32 * 6)()
    assert ctx._lib.jpt_debug_mesh_records(ctx.h, 2, None, None, 0, None, None, 0, info) == E_DEVICE
    ctx.close()


def test_python_wrappers_reach_the_calls(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    with pytest.raises(capi.JptError, match="jpt_scene_update_mesh failed .*host-only"):
        ctx.update_mesh(2, _deformed(sc.meshes[2]))
    g = host.GeometryGroup3D(_small_scene(), capi.BUILD_SAH_WATERTIGHT)
    g.build(host.Context(-1))
    g.scene.meshes[2] = _deformed(g.scene.meshes[2])
    with pytest.raises(capi.JptError, match="jpt_scene_update_mesh failed .*host-only"):
        g.update_mesh(2)
    g2 = host.GeometryGroup3D(_small_scene(), capi.BUILD_SAH)
    g2.build(host.Context(-1))
    with pytest.raises(capi.JptError, match="jpt_scene_update_mesh failed \\(-4\\)"):
        g2.update_mesh(2, _deformed(g2.scene.meshes[2]))
    assert hasattr(host.MultiContext, "update_mesh")
    assert capi.lib().jpt_multi_update_mesh(None, 0, None, 0) == E_INVALID
    ctx.close()


_CPP = r"""
#include <cstdio>
#include <stdexcept>
#include "jpt_host.hpp"
using namespace jpt_host;

static ArrayMesh tetra(float s)
{
    ArrayMesh m;
    Surface x;
    x.vertices = {0, 0, 0, s, 0, 0, 0, s, 0, 0, 0, s};
    x.normals = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    x.uvs = {0, 0, 1, 0, 0, 1, 1, 1};
    x.indices = {0, 1, 2, 0, 1, 3, 0, 2, 3, 1, 2, 3};
    m.surfaces.push_back(x);
    return m;
}

int main(int argc, char** argv)
{
    const int builder = argc > 1 ? atoi(argv[1]) : JPT_BUILD_SAH_WATERTIGHT;
    jpt_ctx* ctx = nullptr;
    if (jpt_create(JPT_DEVICE_HOST_ONLY, &ctx) != JPT_OK) return 2;
    ArrayMesh mesh = tetra(1.0f), other = tetra(2.0f);
    MeshInstance3D node;
    node.mesh = &mesh;
    GeometryGroup3D g;
    g.builder = builder;
    g.add_child(node);
    g.build(ctx);
    for (float& v : mesh.surfaces[0].vertices) v *= 1.5f;
    try {
        g.update_mesh(&mesh);
        std::printf("updated\n");
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
    }
    try {
        g.update_mesh(&other);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
    }
    jpt_destroy(ctx);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_update(hiplib, tmp_path_factory):
    d = tmp_path_factory.mktemp("cpp_mesh")
    src, exe = d / "update_mesh.cpp", str(d / "update_mesh")
    src.write_text(_CPP)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L", libdir, "-ljpt_hip", "-Wl,-rpath," + libdir])
    return exe


def test_cpp_geometry_group_update_mesh_reaches_the_call(cpp_update):
    out = subprocess.run([cpp_update, str(capi.BUILD_SAH_WATERTIGHT)], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert lines[0].startswith("error: jpt_scene_update_mesh") and "host-only" in lines[0], out
    assert "not part of the last build()" in lines[1], out
    out = subprocess.run([cpp_update, str(capi.BUILD_SAH)], capture_output=True, text=True, check=True).stdout
    assert "reach records" in out.splitlines()[0], out
