"""FBX node hierarchies are flattened on import, as the reference's importer does (aiProcess_PreTransformVertices,
libs/DXRFramework/RtModel.cpp:26): rt_fbx_read against tests/fbx_hierarchy_tools.py's independent numpy float64 evaluation of files
its writer emits -- parent chains, pre / post rotations, pivots and offsets, every Euler RotationOrder, geometric transforms, non-mesh
nodes, instanced geometry, InheritType -- and the refusals, each naming its cause.  CPU only: no device is opened.

Tolerance: the two sides are separate float64 products, so a coordinate can fall on either side of a float32 rounding boundary: one
float32 ulp at the largest absolute coordinate for positions, one at 1.0 for the unit normals.  Indices are exact."""
import numpy as np
import pytest

import fbx_hierarchy_tools as H

CASES = H.cases()
RT_ERR_IO, RT_ERR_UNSUPPORTED = -3, -6                            # include/dxr_amd_types.h


def flat(v):
    return np.concatenate([v["position"], v["normal"]], 1)


@pytest.mark.parametrize("version,compress", [(7500, True), (7400, False)])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fbx_hierarchy_is_flattened(capi, tmp_path, case, version, compress):
    geoms, models = CASES[case]
    path = str(tmp_path / (case + ".fbx"))
    H.write(path, geoms, models, version=version, compress=compress)
    want_v, want_i = H.evaluate(path)
    v, i = capi.fbx_read(path)
    got = flat(v)
    n_meshes = sum(len(m.get("geoms", ())) for m in models)
    assert want_i.shape == (12 * n_meshes, 3)
    assert i.shape == want_i.shape and np.array_equal(i, want_i)
    assert got.shape == want_v.shape
    big = np.abs(want_v[:, :3]).max()
    assert 1.0 <= big <= 16.0                                     # coordinates O(1 - 10): the bound below is tight
    perr = np.abs(got[:, :3].astype(np.float64) - want_v[:, :3]).max()
    nerr = np.abs(got[:, 3:].astype(np.float64) - want_v[:, 3:]).max()
    print("%s: max |coordinate| %g, position error %g (bound %g), normal error %g (bound %g)" % (
        case, big, perr, np.spacing(np.float32(big)), nerr, np.spacing(np.float32(1.0))))
    assert perr <= np.spacing(np.float32(big))
    assert nerr <= np.spacing(np.float32(1.0))
    # the evaluation is not the identity: the hierarchy moved the mesh
    plain = np.concatenate([np.asarray(g["positions"]) for g in geoms])
    assert not np.array_equal(np.unique(got[:, :3], axis=0), np.unique(plain.astype(np.float32), axis=0))


def test_instanced_geometry_is_emitted_once_per_model_in_connection_order(capi, tmp_path):
    """(g) in detail: 24 triangles, the first 12 under the first connected Model, and the two copies share no vertex."""
    geoms, models = CASES["g_instanced_geometry"]
    path = str(tmp_path / "g.fbx")
    H.write(path, geoms, models)
    v, i = capi.fbx_read(path)
    assert i.shape == (24, 3)
    first, second = v["position"][np.unique(i[:12])], v["position"][np.unique(i[12:])]
    assert first[:, 0].max() < 0.0 < second[:, 0].min()           # translations -3 and +3 in x
    assert i[:12].max() < i[12:].min()


def test_geometry_without_a_model_and_flat_files_are_unchanged(capi, tmp_path):
    """A Geometry connected to no Model keeps the identity; a Model with only identity factors gives the file's own bits."""
    g = H.box()
    path = str(tmp_path / "loose.fbx")
    H.write(path, [g, g], [dict(parent=None, geoms=[1], props={"PreRotation": (0.0, 0.0, 0.0), "GeometricScaling": (1.0, 1.0, 1.0), "InheritType": 1,
                                                                 "RotationPivot": (0.0, 0.0, 0.0), "RotationOrder": 4})])
    v, i = capi.fbx_read(path)
    assert i.shape == (24, 3)
    a, b = flat(v)[:v.shape[0] // 2], flat(v)[v.shape[0] // 2:]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(np.unique(a[:, :3], axis=0), np.unique(g["positions"].astype(np.float32), axis=0))


def _chain(n, leaf_props=None, props=None):
    models = [dict(cls="Null", parent=(k - 1 if k else None), props=dict(props or {})) for k in range(n - 1)]
    models.append(dict(parent=(n - 2 if n > 1 else None), geoms=[0], props=dict(leaf_props or {})))
    return models


REFUSALS = {
    "spheric_rotation_order": (_chain(2, {"RotationOrder": 6, "Lcl Rotation": (10.0, 20.0, 30.0)}), "RotationOrder", RT_ERR_UNSUPPORTED),
    "spheric_rotation_order_on_an_ancestor": (_chain(3, props={"RotationOrder": 6}), "RotationOrder", RT_ERR_UNSUPPORTED),
    "inherit_type_2_under_a_scaled_parent": (_chain(2, {"InheritType": 2}, {"Lcl Scaling": (2.0, 1.0, 1.0)}), "InheritType", RT_ERR_UNSUPPORTED),
    "inherit_type_0_under_a_scaled_grandparent": ([dict(cls="Null", parent=None, props={"Lcl Scaling": (1.0, 1.0, 3.0)}),
                                                   dict(cls="Null", parent=0, props={}),
                                                   dict(parent=1, geoms=[0], props={"InheritType": 0})], "InheritType", RT_ERR_UNSUPPORTED),
    "parent_cycle": ([dict(cls="Null", parent=1), dict(cls="Null", parent=0), dict(parent=0, geoms=[0])], "cycle", RT_ERR_IO),
    "self_parent": ([dict(parent=0, geoms=[0])], "cycle", RT_ERR_IO),
    "chain_of_300": (_chain(300, props={"Lcl Translation": (0.01, 0.0, 0.0)}), "deeper than 256", RT_ERR_IO),
    "two_parents": ([dict(cls="Null", parent=None), dict(cls="Null", parent=None), dict(parent=[0, 1], geoms=[0])], "more than one parent", RT_ERR_IO),
    "singular_chain": (_chain(3, props={"Lcl Scaling": (1.0, 0.0, 1.0)}), "singular", RT_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_fbx_hierarchy_refusals_name_their_cause(capi, tmp_path, case):
    models, match, code = REFUSALS[case]
    path = str(tmp_path / (case + ".fbx"))
    H.write(path, [H.box()], models)
    with pytest.raises(capi.RtError, match=match) as e:
        capi.fbx_read(path)
    assert e.value.code == code


def test_a_chain_of_256_is_still_read(capi, tmp_path):
    """The depth limit is 256 nodes: that chain loads, and its 255 translations add up."""
    path = str(tmp_path / "deep.fbx")
    H.write(path, [H.box()], _chain(256, props={"Lcl Translation": (0.03125, 0.0, 0.0)}))
    v, i = capi.fbx_read(path)
    want_v, want_i = H.evaluate(path)
    assert np.array_equal(i, want_i) and np.array_equal(v["position"], want_v[:, :3])      # (dyadic steps: both sums are exact)
    assert np.abs(v["normal"].astype(np.float64) - want_v[:, 3:]).max() <= np.spacing(np.float32(1.0))
    assert v["position"][:, 0].max() == np.float32(1.0 + 255 * 0.03125)
