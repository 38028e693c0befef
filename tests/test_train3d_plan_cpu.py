"""CPU: the host plan of vx_train_patches_3d (values_amd/csrc/train3d_plan.h) as a stand-alone program under ASan + UBSan
(tests/train3d_plan_host.cpp; no sanitizer runtime in this process): every refusal, and the lane decomposition over the
shape matrix of tests/test_gpu_trainpatches3d.py -- every output voxel covered exactly once, from the source element
numpy's crop-and-flip names, no source index outside the crop."""
import os
import subprocess

from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
PATCHES = [(1, 1, 1), (2, 3, 1), (3, 5, 6), (4, 4, 4), (5, 5, 5), (7, 2, 9), (8, 8, 8)]
VOLUMES = [(9, 7, 13), (8, 8, 8), (5, 6, 21)]


def test_host_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "train3d_plan_host")
    build_host_program(os.path.join(ROOT, "tests", "train3d_plan_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "BAD-" not in res.stdout, res.stdout
    lines = [ln.split() for ln in res.stdout.splitlines()]
    codes = {ln[0]: int(ln[1]) for ln in lines if ln[0] != "cover"}
    want = {"ok": 0, "ok_no_seg": 0, "ok_below_2_32": 0, "ok_seg_u8_odd": 0, "ok_max": 0,
            "null_table": E_NULL, "null_data": E_NULL, "null_status": E_NULL, "null_workspace": E_NULL, "null_image": E_NULL,
            "n_zero": E_SHAPE, "n_over": E_SHAPE, "n_negative": E_SHAPE, "p_zero": E_SHAPE, "dim_zero": E_SHAPE, "crop_past": E_SHAPE,
            "crop_before": E_SHAPE, "volume_small": E_SHAPE, "p_2_32": E_SHAPE, "var_negative": E_SHAPE, "var_order": E_SHAPE,
            "var_nan": E_SHAPE,
            "kind_image": E_DTYPE, "kind_image_neg": E_DTYPE, "kind_label": E_DTYPE, "flags_high": E_DTYPE, "flags_neg": E_DTYPE,
            "label_flags": E_DTYPE, "law": E_DTYPE,
            "align_data": E_ALIGN, "align_seg": E_ALIGN, "align_sigma": E_ALIGN, "align_status": E_ALIGN, "align_image": E_ALIGN,
            "align_label": E_ALIGN, "align_workspace": E_ALIGN, "workspace_short": E_WORKSPACE}
    assert codes == want
    # one "cover" line per (patch, volume that holds it) and one for the volume equal to the patch; lanes = items * P0 * P1 * ceil(P2 / 4)
    cover = [ln for ln in lines if ln[0] == "cover"]
    expect = []
    for P in PATCHES:
        expect += ["x".join(map(str, P)) for V in VOLUMES + [P] if all(d >= p for d, p in zip(V, P))]
    assert [ln[1] for ln in cover] == expect
    for ln in cover:
        P = [int(v) for v in ln[1].split("x")]
        assert int(ln[2]) == 40 and int(ln[3]) == int(ln[2]) * P[0] * P[1] * ((P[2] + 3) // 4)
