"""The mesh voxeliser on the device (values_amd/csrc/voxelize.hip): everything is `==` to the host mirror
(values_amd/stl.py), volume and odd_columns alike.  The kernel's tile is a row of 64 columns, a mask word 64 k and a step 256
triangles of one mesh: the sphere at 70 crosses a tile edge in x and in y, has two mask words and a partial last tile;
both spheres hold more triangles than one step, the cube fewer."""
import json
import os

import numpy as np
import pytest

from tests import voxel_ref as vr

pytestmark = pytest.mark.gpu

GUARD = 1024          # floats before and after `out`
SENTINEL = -7.0


def run_device(meshes, resolution, out=None):
    """-> (volume as numpy, odd_columns, the guarded buffer): the C entry called on a view with guard regions on both sides"""
    import torch
    from values_amd import stl
    obj = stl.MeshObject(meshes)
    _, _, dims = stl.voxel_grid(meshes, resolution)
    zyx = (int(dims[2]), int(dims[1]), int(dims[0]))
    n = zyx[0] * zyx[1] * zyx[2]
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n].view(zyx)
    got, odd = stl.voxelize_device_info(obj, resolution, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    return host[GUARD:GUARD + n].reshape(zyx), int(odd.cpu()[0]), buf


CASES = [("cube", 1), ("cube", 2), ("cube", 3), ("cube", 13),
         ("bipyramid", 4), ("bipyramid", 8), ("bipyramid", 16),
         ("slab", 10), ("slab", 16),
         ("sphere", 7), ("sphere", 13), ("sphere", 70),
         ("subdivided_sphere", 33)]


@pytest.mark.parametrize("name,resolution", CASES)
def test_device_equals_the_mirror(name, resolution):
    mesh = getattr(vr, name)()
    want, want_odd = vr.mirror(name, [mesh], resolution)
    got, odd, _ = run_device([mesh], resolution)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want) and odd == want_odd == 0
    assert want.any()
    if name.endswith("sphere"):
        assert len(mesh) > 256          # more triangles than one LDS step
    if (name, resolution) == ("sphere", 70):
        assert want.shape == (70, 70, 70) and 0 < want.mean() < 1


def test_two_meshes_labels_and_overwrite_order():
    cube, small = vr.cube(), vr.half_sphere()
    want, want_odd = vr.mirror("cube+half", [cube, small], 24)
    got, odd, _ = run_device([cube, small], 24)
    assert np.array_equal(got, want) and odd == want_odd == 0
    assert set(np.unique(got)) == {1.0, 2.0}
    want, _ = vr.mirror("half+cube", [small, cube], 24)
    got, odd, _ = run_device([small, cube], 24)
    assert np.array_equal(got, want) and (got == 2).all() and odd == 0


def test_open_cube_count_and_volume():
    from values_amd import stl
    mesh = vr.open_cube()
    want, want_odd = vr.mirror("open_cube", [mesh], 9)
    got, odd, _ = run_device([mesh], 9)             # nothing raised at the C level
    assert want_odd > 0 and odd == want_odd and np.array_equal(got, want)
    with pytest.raises(ValueError, match=str(want_odd)):
        stl.voxelize_device([mesh], 9)
    loose = stl.voxelize_device([mesh], 9, strict=False)
    assert np.array_equal(loose.cpu().numpy(), want)


def test_mesh_object_keeps_one_device_copy_of_the_triangles():
    import torch
    from values_amd import stl
    fn = stl.mesh_object([vr.SPHERE, vr.CUBE], device_io=True)
    a = fn(11)
    tris = fn.device_triangles(a.device)
    b = fn(20)
    assert fn.device_triangles(b.device) is tris and tris.shape == (972, 3, 3) and len(fn._device_tris) == 1
    assert isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32
    for t, r in ((a, 11), (b, 20)):
        assert np.array_equal(t.cpu().numpy(), vr.mirror("sphere+cube", [vr.sphere(), vr.cube()], r)[0])


def test_captured_in_a_graph_and_replayed_twice():
    import torch
    from values_amd import stl
    mesh = vr.sphere()
    want, _ = vr.mirror("sphere", [mesh], 13)
    obj = stl.MeshObject([mesh])
    obj.device_triangles(torch.device("cuda", torch.cuda.current_device()))      # uploaded before the capture
    out = torch.full((13, 13, 13), SENTINEL, dtype=torch.float32, device="cuda")
    odd = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one linear stream: two kernel nodes, no parallel branches
        stl.voxelize_device_info(obj, 13, out=out, odd=odd)
    results = []
    for _ in range(2):
        out.fill_(SENTINEL)
        odd.fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), int(odd.cpu()[0])))
    for vol, n_odd in results:
        assert np.array_equal(vol, want) and n_odd == 0


def tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(dirpath, f), root)] = os.path.join(dirpath, f)
    return out


def test_config_device_route_equals_the_host_route(tmp_path):
    from values_amd import generate_toy_dataset_from_config, nifti
    save = str(tmp_path / "imagesTr")            # both routes write into the SAME save_path: the JSON holds it
    generate_toy_dataset_from_config(vr.CASE_1_TRAIN, save_path=save, device_io=False)
    host = str(tmp_path / "host")
    os.rename(save, host)
    generate_toy_dataset_from_config(vr.CASE_1_TRAIN, save_path=save, device_io=True)
    th, td = tree(host), tree(save)
    assert sorted(th) == sorted(td) and len(th) == 2 + 2 * 3 + 1
    for rel in sorted(th):
        if rel.endswith(".json"):
            assert open(th[rel], "rb").read() == open(td[rel], "rb").read()
            info = json.load(open(td[rel]))
            assert info["input_files"] == ["ballSphere.stl"] and info["noise"] is False
            continue
        a, _ = nifti.load(th[rel])
        b, _ = nifti.load(td[rel])
        assert a.dtype == b.dtype and a.shape == b.shape == (64, 64, 64)
        assert np.array_equal(a, b), rel
        assert a.any()
