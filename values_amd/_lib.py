"""ctypes binding of libvalues_amd.so (include/values_amd.h).

The HIP library is the product: there is NO CPU or PyTorch fallback.  If the shared object is
missing or a symbol is absent, import of the compute entry points fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VX_LIB_PATH") or os.path.join(_HERE, "libvalues_amd.so")   # VX_LIB_PATH: A/B builds only

VX_F32, VX_F64 = 0, 1
VX_ACT_NONE, VX_ACT_LRELU, VX_ACT_RELU = 0, 1, 2
VX_DROP_NONE, VX_DROP_HASH, VX_DROP_MASK = 0, 1, 2

_p = C.c_void_p
_i = C.c_int
_i32 = C.c_int32
_u32 = C.c_uint32
_i64 = C.c_int64


class ConvArgs(C.Structure):
    _fields_ = [("in_", _p), ("w_packed", _p), ("bias", _p), ("out", _p),
                ("in_pitch", _i32), ("out_pitch", _i32), ("out_coff", _i32),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("Cout", _i32),
                ("act", _i32), ("drop_mode", _i32), ("drop_seed", _u32), ("drop_layer", _u32),
                ("drop_mask", _p), ("stats_partial", _p), ("in_xblk", _i32), ("w_family", _i32),
                ("head_out", _p), ("head_w", _p), ("head_b", _p), ("head_dst", _p), ("head_flip", _p),
                ("head_C", _i32),
                ("in_mean", _p), ("in_rstd", _p), ("in_drop_mode", _i32), ("in_drop_seed", _u32), ("in_drop_layer", _u32),
                ("in_repeat", _i32), ("out_xblk", _i32), ("out_half", _i32), ("range_flag", _p), ("seed_dev", _p),
                ("up_in", _p), ("up_w", _p), ("up_b", _p), ("up_pitch", _i32), ("pool_out", _p), ("pool_flags", _p),
                ("in_split", _i32), ("out_f16", _i32), ("in_f16", _i32),
                ("out_split", _i32), ("up_split", _i32), ("up_fused", _p), ("in_pool_flags", _p),
                ("acc_in", _p), ("acc_pitch", _i32), ("out_planar", _i32), ("in_planar", _i32), ("products", _i32)]


class NormArgs(C.Structure):
    _fields_ = [("x", _p), ("x_pitch", _i32), ("mean", _p), ("rstd", _p),
                ("out", _p), ("out_pitch", _i32), ("out_coff", _i32),
                ("pool_out", _p), ("pool_pitch", _i32),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("C", _i32),
                ("act", _i32), ("drop_mode", _i32), ("drop_seed", _u32), ("drop_layer", _u32), ("drop_mask", _p),
                ("out_xblk", _i32), ("out_half", _i32), ("x_xblk", _i32), ("x_half", _i32), ("seed_dev", _p),
                ("range_flag", _p)]


class StatSrc(C.Structure):
    """vx_stat_src: a streaming pass reduces the producing conv's statistics partials itself (round 5)."""
    _fields_ = [("stats_partial", _p), ("tiles", _i32), ("eps", C.c_float), ("count", _i64), ("mean_out", _p), ("rstd_out", _p)]


class NormRouteInfo(C.Structure):
    """vx_norm_route_info: the launch geometry and index decode vx_norm_act_drop_pool_route reports."""
    _fields_ = [("grid_x", _i32), ("grid_y", _i32), ("per_sample", _u32), ("magic_pw", _u32), ("magic_c4", _u32), ("magic_rh", _u32)]


class ConvTArgs(C.Structure):
    _fields_ = [("in_", _p), ("in_pitch", _i32), ("w_packed", _p), ("bias", _p),
                ("out", _p), ("out_pitch", _i32), ("out_coff", _i32),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("Cout", _i32),
                ("act", _i32), ("drop_mode", _i32), ("drop_seed", _u32), ("drop_layer", _u32), ("drop_mask", _p),
                ("out_xblk", _i32), ("out_half", _i32), ("range_flag", _p), ("seed_dev", _p)]


class ConvTRouteInfo(C.Structure):
    """vx_convT_route_info: the grid vx_convT_k2s2_route reports."""
    _fields_ = [("grid_x", _i32), ("grid_y", _i32)]


class Conv2dArgs(C.Structure):
    _fields_ = [("in_", _p), ("in_pitch", _i32), ("w_packed", _p), ("bias", _p),
                ("out", _p), ("out_pitch", _i32), ("out_coff", _i32),
                ("N", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("Cout", _i32), ("KS", _i32), ("S", _i32),
                ("stats_partial", _p), ("w_family", _i32),
                ("in_scale", _p), ("in_shift", _p), ("in_cpitch", _i32), ("in_group_images", _i32), ("in_relu", _i32),
                ("out_scale", _p), ("out_shift", _p), ("out_add", _p), ("out_add_pitch", _i32), ("out_act", _i32)]


class Conv2dRouteInfo(C.Structure):
    """vx_conv2d_route_info: the launch geometry vx_conv2d_route reports."""
    _fields_ = [("nchunks", _i32), ("w_all", _i32), ("lds_bytes", _i32), ("grid_x", _i32), ("grid_y", _i32)]


class BnAffineItem(C.Structure):
    """vx_bn_affine_item: one BatchNorm layer of vx_bn_running_affine (running statistics -> scale / shift rows)."""
    _fields_ = [("gamma", _p), ("beta", _p), ("running_mean", _p), ("running_var", _p), ("scale", _p), ("shift", _p),
                ("C", _i32), ("cpitch", _i32)]


class AffineArgs(C.Structure):
    _fields_ = [("x", _p), ("x_pitch", _i32), ("scale", _p), ("shift", _p), ("add", _p), ("add_pitch", _i32),
                ("out", _p), ("out_pitch", _i32), ("out_coff", _i32),
                ("N", _i32), ("H", _i32), ("W", _i32), ("C", _i32), ("OH", _i32), ("OW", _i32),
                ("act", _i32), ("drop_mode", _i32), ("drop_seed", _u32), ("drop_layer", _u32), ("drop_mask", _p),
                ("group_images", _i32)]


class FuseTerm(C.Structure):
    _fields_ = [("x", _p), ("x_pitch", _i32), ("H", _i32), ("W", _i32), ("scale", _p), ("shift", _p)]


class FuseArgs(C.Structure):
    _fields_ = [("term", FuseTerm * 4), ("nterms", _i32), ("out", _p), ("out_pitch", _i32),
                ("N", _i32), ("OH", _i32), ("OW", _i32), ("C", _i32), ("act", _i32), ("group_images", _i32)]


class Config(C.Structure):
    """vx_config (include/values_amd.h): kernel-family selection and tuning knobs, read once from VX_* variables."""
    _fields_ = [(n, _i32) for n in (
        "conv_fp32", "s16_no_prenorm", "s16_no_xp8", "s16_skip_raw", "no_head_fusion", "s16_no_upfuse", "s16_no_poolfuse",
        "storage16", "s16_generic", "s16_no_zc16", "s16_no_halves", "s16_no_deep", "s16_no_l1dma", "c2s_no_wide", "c2s_no_oct")]
    # switches vx_version 700 retired (their launch sequences were measured slower; the default is the only path left): they
    # read as 0 and take 0, so code that resets them keeps working, and asking for the retired path is an error
    RETIRED = ("s16_no_upcompose", "s16_no_upsplit", "s16_no_poolfin", "s16_no_presplit", "s16_no_dbplain")


def _retired_field(name):
    def put(self, v):
        if v:
            raise ValueError(f"vx_config.{name} was retired in 0.7.0: the default data flow is the only one")
    return property(lambda self: 0, put)


for _n in Config.RETIRED:
    setattr(Config, _n, _retired_field(_n))


class UncOutputs(C.Structure):
    _fields_ = [("mean_prob", _p), ("pred_entropy", _p), ("exp_entropy", _p), ("mutual_info", _p), ("variance", _p),
                ("argmax", _p), ("sample_argmax", _p), ("in_count", _p), ("out_count", _p)]


class UNet3DWeights(C.Structure):
    _fields_ = [("conv_w", _p * 18), ("conv_b", _p * 18), ("up_w", _p * 4), ("up_b", _p * 4),
                ("final_w", _p), ("final_b", _p), ("F", _i32), ("num_classes", _i32), ("conv_family", _i32 * 18),
                ("in_channels", _i32), ("no_instancenorm", _i32), ("up_fused", _p), ("split_w", _p * 2), ("split_family", _i32), ("up3_zc16", _p), ("up3_fused", _p)]


class UNet3DRun(C.Structure):
    _fields_ = [("x", _p), ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("repeat", _i32),
                ("src", _p), ("flip", _p), ("dst", _p), ("drop_mode", _i32), ("seed", _u32),
                ("masks", _p * 17), ("logits", _p), ("workspace", _p), ("workspace_bytes", C.c_size_t),
                ("range_flag", _p), ("seed_dev", _p)]


VX_NIFTI_COPY, VX_NIFTI_PROB, VX_NIFTI_MEAN_PROB, VX_NIFTI_ARGMAX, VX_NIFTI_ARGMAX_MEAN = 0, 1, 2, 3, 4


class NiftiItem(C.Structure):
    """vx_nifti_item: one NIfTI payload (header + Fortran-order voxels) of the device results writer."""
    _fields_ = [("src", _p), ("count", _p), ("dst_off", _i64), ("kind", _i32), ("src_dtype", _i32), ("esize", _i32),
                ("T", _i32), ("C", _i32), ("t", _i32), ("c", _i32), ("X", _i32), ("Y", _i32), ("Z", _i32),
                ("header", C.c_uint8 * 352)]


class GzItem(C.Structure):
    """vx_gz_item: one gzip member to encode (device source, n bytes, slot offset in dst, match-finder stride hints)."""
    _fields_ = [("src", _p), ("n", _i64), ("dst_off", _i64), ("stride_hint", _i32 * 3), ("pad", _i32)]


class PngItem(C.Structure):
    """vx_png_item: one (H, W) uint8 label mask to encode as an RGB PNG (device labels, optional device ignore map)."""
    _fields_ = [("labels", _p), ("ignore", _p), ("H", _i32), ("W", _i32)]


class PngRgbItem(C.Structure):
    """vx_png_rgb_item: one (H, W, 3) uint8 RGB image to encode as an RGB PNG (device pixels)."""
    _fields_ = [("rgb", _p), ("H", _i32), ("W", _i32)]


class InflateItem(C.Structure):
    """vx_inflate_item: one compressed stream (device src, src_n bytes) and its output window dst[dst_off, +dst_cap)."""
    _fields_ = [("src", _p), ("src_n", _i64), ("dst_off", _i64), ("dst_cap", _i64), ("format", _i32), ("pad", _i32)]


VX_INFLATE_GZIP, VX_INFLATE_ZLIB, VX_INFLATE_RAW = 0, 1, 2
INFLATE_STATUS = ("ok", "truncated", "bad header", "bad block type", "invalid code lengths", "bad symbol",
                  "distance beyond the output start", "output capacity reached", "checksum mismatch", "ISIZE mismatch",
                  "trailing bytes", "stored block length mismatch", "preset dictionary")
VX_INFLATE_CAPACITY = 7


class NiftiDecItem(C.Structure):
    """vx_nifti_dec_item: the voxels of one decoded NIfTI payload to a C-order array (out_dtype -1: the file's type)."""
    _fields_ = [("src", _p), ("src_n", _i64), ("vox_offset", _i64), ("dst", _p), ("dst_n", _i64), ("ndim", _i32),
                ("dims", _i32 * 7), ("code", _i32), ("big_endian", _i32), ("out_dtype", _i32), ("pad", _i32),
                ("slope", C.c_double), ("inter", C.c_double)]


class PngUnfilterItem(C.Structure):
    """vx_png_unfilter_item: one inflated PNG scanline stream (device src, src_n bytes) to reconstruct into dst."""
    _fields_ = [("src", _p), ("src_n", _i64), ("dst", _p), ("H", _i32), ("W", _i32), ("bpp", _i32), ("pad", _i32)]


VX_PNG_OK, VX_PNG_BAD_FILTER, VX_PNG_BAD_SIZE = 0, 1, 2
PNG_STATUS = ("ok", "filter byte above 4", "stream size is not H (1 + W bpp)")


class TiffLzwItem(C.Structure):
    """vx_tiff_lzw_item: one LZW strip (device src, src_n bytes) and its output window dst[dst_off, +dst_cap)."""
    _fields_ = [("src", _p), ("src_n", _i64), ("dst_off", _i64), ("dst_cap", _i64)]


class TiffUnpredictItem(C.Structure):
    """vx_tiff_unpredict_item: `rows` float32 rows of W samples (device src -> dst) whose predictor (2 / 3) is undone."""
    _fields_ = [("src", _p), ("dst", _p), ("rows", _i32), ("W", _i32), ("predictor", _i32), ("pad", _i32)]


VX_LZW_OK, VX_LZW_TRUNCATED, VX_LZW_BAD_CODE = 0, 1, 2
LZW_STATUS = ("ok", "truncated", "bad code")
VX_LZW_NO_ROOM = 3   # vx_tiff_lzw_encode alone: the item's window is smaller than its strip


VX_AGG_IMAGE, VX_AGG_THRESHOLD, VX_AGG_PATCH = 0, 1, 2
VX_AGG_MAX_SPECS, VX_AGG_MAX_ITEMS = 8, 4096


class AggItem(C.Structure):
    """vx_agg_item: one device map [D][H][W] (a 2D map: D = 1) of VX_F32 / VX_F64 for vx_aggregate_batched."""
    _fields_ = [("map", _p), ("dtype", _i32), ("D", _i32), ("H", _i32), ("W", _i32)]


class AggSpec(C.Structure):
    """vx_agg_spec: one aggregation of a vx_aggregate_batched call (kind VX_AGG_*; patch for PATCH, thr for THRESHOLD)."""
    _fields_ = [("kind", _i32), ("pd", _i32), ("ph", _i32), ("pw", _i32), ("thr", C.c_double)]


VX_EM_MAX_ITEMS = 4096


class EmItem(C.Structure):
    """vx_em_item: one image of vx_platt_sums_batched / vx_calib_bins_batched: device map [nvox] (VX_F32 / VX_F64), int32
    reference segmentations [R][nvox] and mean prediction [nvox]."""
    _fields_ = [("unc", _p), ("ref", _p), ("pred", _p), ("nvox", _i64), ("dtype", _i32), ("R", _i32)]


class NccItem(C.Structure):
    """vx_ncc_item: one map pair of vx_ncc_batched; gt is a map (gt_R = 0) or gt_R int32 label volumes [gt_R][n_gt]."""
    _fields_ = [("gt", _p), ("pred", _p), ("n_gt", _i64), ("n_pred", _i64), ("gt_dtype", _i32), ("pred_dtype", _i32),
                ("gt_R", _i32), ("reserved", _i32)]


VX_SELECT_MAX_ITEMS = 65536
VX_COUNT_B1, VX_COUNT_B2, VX_COUNT_B4, VX_COUNT_B8, VX_COUNT_F32, VX_COUNT_F64 = range(6)
VX_SELECT_OK, VX_SELECT_NAN = 0, 1


class CountItem(C.Structure):
    """vx_count_item: one device array of n elements of kind VX_COUNT_* for vx_count_nonzero_batched."""
    _fields_ = [("ptr", _p), ("n", _i64), ("kind", _i32), ("reserved", _i32)]


class SelectItem(C.Structure):
    """vx_select_item: one device array of n VX_F32 / VX_F64 elements for vx_select_segments."""
    _fields_ = [("ptr", _p), ("n", _i64), ("dtype", _i32), ("reserved", _i32)]


VX_PREP_U8, VX_PREP_I8, VX_PREP_U16, VX_PREP_I16, VX_PREP_U32, VX_PREP_I32, VX_PREP_F32, VX_PREP_F64 = range(8)
VX_PREP_ZSCORE, VX_PREP_COPY = 0, 1
VX_PREP_OWN = -1


class PrepItem(C.Structure):
    """vx_prep_item: one device array of n elements of kind VX_PREP_* for vx_volume_stats_batched."""
    _fields_ = [("ptr", _p), ("n", _i64), ("kind", _i32), ("reserved", _i32)]


class PrepPadItem(C.Structure):
    """vx_prep_pad_item: one volume (ZSCORE) or label (COPY) of vx_zscore_pad_batched: the source box dims at pad_below of
    the output box out_dims, its row of the statistics."""
    _fields_ = [("src", _p), ("dst", _p), ("dims", _i32 * 3), ("out_dims", _i32 * 3), ("pad_below", _i32 * 3),
                ("kind", _i32), ("out_dtype", _i32), ("mode", _i32), ("stats_row", _i32), ("reserved", _i32)]


VX_P2D_IMAGE, VX_P2D_LABEL_IDS, VX_P2D_LABEL_COLOR = 0, 1, 2


class P2dItem(C.Structure):
    """vx_p2d_item: one decoded image or label file of vx_crop_resize_batched: the source [H][W][bpp] (palette: device
    256 x 3 bytes for an indexed file, else null), the crop box, the even factor, the mode and its outputs."""
    _fields_ = [("src", _p), ("palette", _p), ("H", _i32), ("W", _i32), ("bpp", _i32), ("y0", _i32), ("x0", _i32),
                ("crop_h", _i32), ("crop_w", _i32), ("factor", _i32), ("mode", _i32), ("reserved", _i32), ("out_rgb", _p),
                ("out_ids", _p)]


class P2dTables(C.Structure):
    """vx_p2d_tables: the device tables of vx_crop_resize_batched (id -> train id, train id -> colour, colour -> train id)."""
    _fields_ = [("id2trainid", _p), ("trainid2color", _p), ("color2trainid", _p), ("n_color", _i32), ("default_id", _i32)]


VX_LSWITCH_MAX_R, VX_LSWITCH_MAX_ROWS = 31, 8


class LswitchItem(C.Structure):
    """vx_lswitch_item: one label map [H][W] of vx_label_switch_batched (kind VX_COUNT_B1 .. B8), its rater planes
    [R][H * W] uint8 and / or its variance map [W][H] float32, and the image's split index."""
    _fields_ = [("labels", _p), ("refs", _p), ("variance", _p), ("H", _i32), ("W", _i32), ("kind", _i32), ("index", _u32)]


class LswitchRow(C.Structure):
    """vx_lswitch_row: one label switch from -> to, drawn with thr = (uint32)(p * 2^24)."""
    _fields_ = [("from_", _i32), ("to", _i32), ("thr", _u32)]


VX_COMPOSITE_MAX_LABELS = 1 << 20
VX_LABEL_SIGNED = 1


class Gather3dItem(C.Structure):
    """vx_gather3d_item: one crop of vx_gather_patches_3d: the volume src [dims] of kind VX_PREP_* and the crop's origin."""
    _fields_ = [("src", _p), ("kind", _i32), ("dims", _i32 * 3), ("origin", _i32 * 3), ("reserved", _i32)]


VX_TRAIN3D_MIRROR0, VX_TRAIN3D_MIRROR1, VX_TRAIN3D_MIRROR2, VX_TRAIN3D_NOISE = 1, 2, 4, 8


class Train3dItem(C.Structure):
    """vx_train3d_item: one sample of vx_train_patches_3d: image (VX_PREP_*) and label (VX_COUNT_B1 .. B8, flags 0 or
    VX_LABEL_SIGNED; null: none) of one case, the crop's origin, flags (bits 0-2 mirror axis 0 / 1 / 2, bit 3 noise) and the
    global sample index that keys the noise stream."""
    _fields_ = [("image", _p), ("label", _p), ("image_kind", _i32), ("label_kind", _i32), ("label_flags", _i32),
                ("dims", _i32 * 3), ("origin", _i32 * 3), ("flags", _i32), ("index", _u32)]


class Acc3dItem(C.Structure):
    """vx_acc3d_item: the destination of one patch of vx_softmax_accumulate_cases: sum [T][C][X][Y][Z], count [X][Y][Z],
    dims = (X, Y, Z) and where the patch lands."""
    _fields_ = [("sum", _p), ("count", _p), ("dims", _i32 * 3), ("origin", _i32 * 3)]


class CompositeLabel(C.Structure):
    """vx_composite_label: one rater file's payload on the device, kind VX_COUNT_B1 .. B8, flags 0 or VX_LABEL_SIGNED."""
    _fields_ = [("ptr", _p), ("kind", _i32), ("flags", _i32)]


class CompositeItem(C.Structure):
    """vx_composite_item: one case of vx_case_composite: image (VX_PREP_*), count map, its raters
    labels[first_label .. first_label + R) and the outputs data f64 / gt_seg f64 [R] / gt u8 [R] (each may be null)."""
    _fields_ = [("image", _p), ("count", _p), ("data", _p), ("gt_seg", _p), ("gt", _p), ("image_kind", _i32),
                ("first_label", _i32), ("R", _i32), ("dims", _i32 * 3)]


VX_MSR_MAX_ITEMS, VX_MSR_MAX_PLANES = 65536, 1 << 22


class MsrItem(C.Structure):
    """vx_msr_item: one image of vx_one_minus_msr_batched: out and the C planes planes[first_plane .. first_plane + C) of n
    VX_F32 / VX_F64 elements each."""
    _fields_ = [("out", _p), ("n", _i64), ("first_plane", _i32), ("C", _i32), ("dtype", _i32), ("reserved", _i32)]


# symbol -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
SIGNATURES = {
    "vx_version": (_i, []),
    "vx_last_error_string": (C.c_char_p, []),
    "vx_last_kernel_name": (C.c_char_p, []),
    "vx_drop_hash_mask": (_i, [_u32, _u32, _i, _i64, _p, _p]),
    "vx_get_config": (_i, [C.POINTER(Config)]),
    "vx_set_config": (_i, [C.POINTER(Config)]),
    "vx_conv3d_k3_family": (_i, [_i, _i]),
    "vx_conv2d_family": (_i, [_i, _i, _i]),
    "vx_unc_reduce": (_i, [_p, _i, _i, _i, _i, _i, _i64, _p, _p, _p, _p, _p, _p, _p]),
    "vx_unc_reduce_ex": (_i, [_p, _i, _i, _i, _i, _i, _i64, C.POINTER(UncOutputs), _p]),
    "vx_unc_stats_accumulate": (_i, [_p, _i, _i, _i, _i64, _p, _p]),
    "vx_unc_stats_finalize": (_i, [_p, _i, _i, _i, _i64, _p, _p, _p, _p, _p, _p]),
    "vx_softmax_planar": (_i, [_p, _i64, _i, _i64, _p, _p]),
    "vx_one_minus_msr": (_i, [_p, _i, _i, _i64, _p, _p]),
    "vx_one_minus_msr_batched_workspace_bytes": (_i64, [_i, _i]),
    "vx_one_minus_msr_batched": (_i, [C.POINTER(MsrItem), _i, C.POINTER(_p), _i, _p, _i64, _p]),
    "vx_conv3d_k3_packed_floats": (_i64, [_i, _i]),
    "vx_pack_conv3d_k3": (_i, [_p, _p, _i, _i, _p]),
    "vx_convT_k2s2_packed_floats": (_i64, [_i, _i]),
    "vx_pack_convT_k2s2": (_i, [_p, _p, _i, _i, _p]),
    "vx_conv3d_k3_tiles": (_i, [_i, _i, _i]),
    "vx_conv3d_k3_tiles_for": (_i, [_i, _i, _i, _i]),
    "vx_conv3d_k3_head_fusable": (_i, [_i, _i]),
    "vx_conv3d_k3_route": (_i, [C.POINTER(ConvArgs), C.c_char_p, _i]),
    "vx_conv3d_k3_prologue_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_upfuse_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_poolfuse_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_presplit_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_poolfin_ok": (_i, [_i, _i]),
    "vx_conv3d_upfused_packed_floats": (_i64, []),
    "vx_pack_conv3d_upfused": (_i, [_p, _p, _p, _p, _p, _p]),
    "vx_pack_conv3d_upfused_zc16": (_i, [_p, _p, _p, _p, _p]),
    "vx_conv3d_upfused_zc16_packed_floats": (_i64, []),
    "vx_pool_finish": (_i, [_p, _p, _p, _p, _p, _i, _i, _i64, _i, _p]),
    "vx_pool_finish_z": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i64, _i, _p]),
    "vx_conv3d_k3_pool_layout": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_skip_prologue_ok": (_i, [_i, _i, _i, _i, _i, _i]),
    "vx_conv3d_k3_acc_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_conv3d_k3_planar_ok": (_i, [_i, _i, _i, _i, _i]),
    "vx_convT_zc16_packed_floats": (_i64, []),
    "vx_pack_convT_zc16": (_i, [_p, _p, _p]),
    "vx_prenorm_split": (_i, [_p, _p, _p, _i, _i64, C.c_float, _p]),
    "vx_zero": (_i, [_p, _i64, _p]),
    "vx_conv3d_k3": (_i, [C.POINTER(ConvArgs), _p]),
    "vx_conv3d_k3_c1_tiles": (_i, [_i, _i, _i]),
    "vx_conv3d_k3_c1": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "vx_pack_input_cl8": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "vx_instnorm_finalize": (_i, [_p, _i, _i, _i, _i64, C.c_float, _p, _p, _p]),
    "vx_norm_act_drop_pool": (_i, [C.POINTER(NormArgs), _p]),
    "vx_norm_act_drop_pool_bcast": (_i, [C.POINTER(NormArgs), _i, _p]),
    "vx_norm_act_drop_pool_stats": (_i, [C.POINTER(NormArgs), C.POINTER(StatSrc), _p]),
    "vx_norm_act_drop_pool_route": (_i, [C.POINTER(NormArgs), _i, C.POINTER(StatSrc), C.c_char_p, _i, C.POINTER(NormRouteInfo)]),
    "vx_prenorm_split_stats": (_i, [_p, C.POINTER(StatSrc), _i, _i64, C.c_float, _p]),
    "vx_pool_finish_z_stats": (_i, [_p, _p, C.POINTER(StatSrc), _p, _i, _i, _i, _i64, _i, _p]),
    "vx_convT_k2s2": (_i, [C.POINTER(ConvTArgs), _p]),
    "vx_convT_k2s2_route": (_i, [C.POINTER(ConvTArgs), C.c_char_p, _i, C.POINTER(ConvTRouteInfo)]),
    "vx_conv1x1_ncdhw": (_i, [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "vx_unet3d_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "vx_unet3d_forward": (_i, [C.POINTER(UNet3DWeights), C.POINTER(UNet3DRun), _p]),
    "vx_unet3d_forward_profiled": (_i, [C.POINTER(UNet3DWeights), C.POINTER(UNet3DRun), _p, _i, C.POINTER(C.c_float),
                                        C.POINTER(C.c_char_p), C.POINTER(_i)]),
    "vx_softmax_accumulate": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vx_aleatoric_sample": (_i, [_p, _p, _u32, _i, _i, _i, _i64, _p, _p, _p]),
    "vx_colorize_u8": (_i, [_p, _p, _i64, _p, _i, _p, _p]),
    "vx_fuse_sum": (_i, [C.POINTER(FuseArgs), _p]),
    "vx_tta_views_2d": (_i, [_p, _i, _p, _p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _i, _i, _i, _i,
                             C.POINTER(C.c_int32), _p, _p]),
    "vx_tta_views_2d_gen": (_i, [_p, _i, _p, _p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _i, _i, _i, _i,
                                 C.POINTER(C.c_int32), _u32, _p, _i64, C.POINTER(C.c_float), _p, _p, _p]),
    "vx_noise_view_3d": (_i, [_p, _p, _i, _i64, _u32, _p, _i64, C.c_float, C.c_float, _i, _p, _p]),
    "vx_count_nonzero_batched_workspace_bytes": (_i64, [_i]),
    "vx_count_nonzero_batched": (_i, [C.POINTER(CountItem), _i, _p, _p, _i64, _p]),
    "vx_select_segments_workspace_bytes": (_i64, [_i]),
    "vx_select_segments": (_i, [C.POINTER(SelectItem), _i, _i64, _p, _p, _p, _i64, _p]),
    "vx_volume_stats_batched_workspace_bytes": (_i64, [C.POINTER(PrepItem), _i]),
    "vx_volume_stats_batched": (_i, [C.POINTER(PrepItem), _i, _p, _p, _i64, _p]),
    "vx_zscore_pad_batched_workspace_bytes": (_i64, [C.POINTER(PrepPadItem), _i]),
    "vx_zscore_pad_batched": (_i, [C.POINTER(PrepPadItem), _i, _p, _p, _i64, _p]),
    "vx_p2d_out_size": (_i, [_i, _i]),
    "vx_crop_resize_batched_workspace_bytes": (_i64, [C.POINTER(P2dItem), _i, C.POINTER(P2dTables)]),
    "vx_crop_resize_batched": (_i, [C.POINTER(P2dItem), _i, C.POINTER(P2dTables), _p, _p, _i64, _p]),
    "vx_label_switch_batched_workspace_bytes": (_i64, [_i, _i]),
    "vx_label_switch_batched": (_i, [C.POINTER(LswitchItem), _i, _i, C.POINTER(LswitchRow), _i, _p, _u32, C.POINTER(C.c_float), _p,
                                     _p, _i64, _p]),
    "vx_gather_patches_3d_workspace_bytes": (_i64, [_i]),
    "vx_gather_patches_3d": (_i, [C.POINTER(Gather3dItem), _i, _p, _i, _i, _i, _p, _i64, _p]),
    "vx_train_patches_3d_workspace_bytes": (_i64, [_i]),
    "vx_train_patches_3d": (_i, [C.POINTER(Train3dItem), _i, _i, _i, _i, _p, _p, _i, _u32, _p, C.c_float, C.c_float, _i, _p, _p, _p,
                                 _i64, _p]),
    "vx_softmax_accumulate_cases_workspace_bytes": (_i64, [_i]),
    "vx_softmax_accumulate_cases": (_i, [_p, _i, _i, _i, _i, _i, _i, C.POINTER(Acc3dItem), _i, _p, _i64, _p]),
    "vx_case_composite_workspace_bytes": (_i64, [_i, _i]),
    "vx_case_composite": (_i, [C.POINTER(CompositeItem), _i, C.POINTER(CompositeLabel), _i, _p, _p, _i64, _p]),
    "vx_toy_embed": (_i, [_p, C.POINTER(_i32), C.POINTER(_i32), C.c_double, _i, _i, _p, C.POINTER(_i32), _p]),
    "vx_gauss_blur_axis_f64": (_i, [_p, _p, C.POINTER(_i32), _i, _p, _i, _p]),
    "vx_count_ge_f64": (_i, [_p, _i64, C.c_double, _p, _p]),
    "vx_order_stats_f64_workspace_bytes": (_i64, [_i]),
    "vx_order_stats_f64_reads": (_i, [_i64, C.POINTER(_i64), _i]),
    "vx_order_stats_f64": (_i, [_p, _i64, C.POINTER(_i64), _i, _p, _p, _p, _i64, _p]),
    "vx_toy_segment": (_i, [_p, _i64, C.POINTER(C.c_double), _i, _p, _p]),
    "vx_toy_noise": (_i, [_p, _i64, _u32, _u32, C.c_double, _p]),
    "vx_voxelize_meshes": (_i, [_p, C.POINTER(_i64), _i, C.POINTER(C.c_double), C.c_double, C.POINTER(_i32), _p, _p, _p]),
    "vx_mask_agreement": (_i, [_p, _i, _i, _i64, _p, _p]),
    "vx_mask_agreement_batched": (_i, [_p, _i, _i, _i, _i64, _i, _p, _p]),
    "vx_soft_metric_workspace_bytes": (_i64, [_i, _i]),
    "vx_soft_metric_sums": (_i, [_p, _p, _i, _i, _i64, _p, _p, _p]),
    "vx_soft_metric_batched_workspace_bytes": (_i64, [_i, _i, _i, _i64]),
    "vx_soft_metric_sums_batched": (_i, [_p, _p, _i, _i, _i, _i64, _p, _p, _p]),
    "vx_val_sums_workspace_bytes": (_i64, [_i, _i, _i64]),
    "vx_val_sums_batched": (_i, [_p, _p, _i, _i, _i64, _i, _p, _p, _i64, _p]),
    "vx_val_aleatoric_sums_workspace_bytes": (_i64, [_i, _i, _i64]),
    "vx_val_aleatoric_sums_batched": (_i, [_p, _p, _u32, _u32, _p, _i, _i, _i, _i64, _i, _p, _p, _i64, _p]),
    "vx_val_ssn_sums_workspace_bytes": (_i64, [_i, _i, _i, _i64]),
    "vx_val_ssn_sums_batched": (_i, [_p, _p, _p, _u32, _u32, _p, _i, _i, _i, _i, _i64, C.c_float, _i, _p, _p, _p, _i64, _p]),
    "vx_val_ssn2d_sums_workspace_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "vx_val_ssn2d_sums_batched": (_i, [_p, _i, _p, _i, _p, _p, _u32, _u32, _p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _i, _p, _p,
                                       _p, _i64, _p]),
    "vx_ssn2d_lowres": (_i, [_p, _i, _p, _i, _p, _u32, _i, _i64, _i, _i, _i, _p, _p, _p]),
    "vx_ssn2d_add_diag": (_i, [_p, _p, _p, _u32, _i, _i, _i64, C.c_float, _p]),
    "vx_softmax_variance": (_i, [_p, _i, _i, _i, _i, _i64, _p, _p]),
    "vx_ssn_sample": (_i, [_p, _p, _p, _u32, _i, _i, _i, _i, _i64, C.c_float, _p, _p]),
    "vx_conv2d_packed_floats": (_i64, [_i, _i, _i]),
    "vx_pack_conv2d": (_i, [_p, _p, _i, _i, _i, _p]),
    "vx_conv2d_tiles": (_i, [_i, _i, _i, _i]),
    "vx_conv2d": (_i, [C.POINTER(Conv2dArgs), _p]),
    "vx_conv2d_route": (_i, [C.POINTER(Conv2dArgs), C.c_char_p, _i, C.POINTER(Conv2dRouteInfo)]),
    "vx_bn_finalize": (_i, [_p, _i, _i, _i64, C.c_float, _p, _p, _p, _p, _p]),
    "vx_bn_finalize_groups": (_i, [_p, _i, _i, _i, _i, _i64, C.c_float, _p, _p, _p, _p, _p]),
    "vx_bn_running_affine": (_i, [_p, _i, C.c_float, _p]),
    "vx_affine_gather": (_i, [C.POINTER(AffineArgs), _p]),
    "vx_bilinear_nchw": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "vx_bilinear_softmax_nchw": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "vx_ncc_batched_workspace_bytes": (C.c_size_t, [C.POINTER(NccItem), _i]),
    "vx_ncc_batched": (_i, [C.POINTER(NccItem), _i, _p, _p, C.c_size_t, _p]),
    "vx_rater_variance": (_i, [_p, _i, _i64, _p, _p]),
    "vx_platt_batched_workspace_bytes": (C.c_size_t, [C.POINTER(EmItem), _i]),
    "vx_platt_sums_batched": (_i, [C.POINTER(EmItem), _i, C.POINTER(C.c_double), _i, _p, _p, C.c_size_t, _p]),
    "vx_calib_batched_workspace_bytes": (C.c_size_t, [C.POINTER(EmItem), _i]),
    "vx_calib_bins_batched": (_i, [C.POINTER(EmItem), _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _p, _p,
                                   C.c_size_t, _p]),
    "vx_aggregate_workspace_bytes": (C.c_size_t, [C.POINTER(AggItem), _i, C.POINTER(AggSpec), _i]),
    "vx_aggregate_batched": (_i, [C.POINTER(AggItem), _i, C.POINTER(AggSpec), _i, _p, _p, C.c_size_t, _p]),
    "vx_nifti_workspace_bytes": (C.c_size_t, [_i]),
    "vx_nifti_payload_bytes": (_i64, [C.POINTER(NiftiItem)]),
    "vx_nifti_payload": (_i, [C.POINTER(NiftiItem), _i, _p, _i64, _p, C.c_size_t, _p]),
    "vx_gzip_bound": (_i64, [_i64]),
    "vx_gzip_workspace_bytes": (C.c_size_t, [C.POINTER(_i64), _i]),
    "vx_gzip_encode": (_i, [C.POINTER(GzItem), _i, _p, _i64, _p, _p, C.c_size_t, _p]),
    "vx_crc32": (_i, [_p, _i64, _p, _p]),
    "vx_png_bound": (_i64, [_i, _i]),
    "vx_png_workspace_bytes": (C.c_size_t, [C.POINTER(PngItem), _i]),
    "vx_png_encode": (_i, [C.POINTER(PngItem), _i, _p, _i, _p, _i64, _p, _p, _p, C.c_size_t, _p]),
    "vx_png_encode_rgb_workspace_bytes": (C.c_size_t, [C.POINTER(PngRgbItem), _i]),
    "vx_png_encode_rgb": (_i, [C.POINTER(PngRgbItem), _i, _p, _i64, _p, _p, _p, C.c_size_t, _p]),
    "vx_inflate_workspace_bytes": (_i64, [_i]),
    "vx_inflate": (_i, [C.POINTER(InflateItem), _i, _p, _i64, _p, _p, _p, _i64, _p]),
    "vx_nifti_decode_workspace_bytes": (_i64, [_i]),
    "vx_nifti_decode": (_i, [C.POINTER(NiftiDecItem), _i, _p, _i64, _p]),
    "vx_png_unfilter_workspace_bytes": (_i64, [_i]),
    "vx_png_unfilter": (_i, [C.POINTER(PngUnfilterItem), _i, _p, _p, _i64, _p]),
    "vx_rgb_to_trainid": (_i, [_p, _i64, _p, _i, _i, _p, _p]),
    "vx_tiff_lzw_workspace_bytes": (_i64, [_i]),
    "vx_tiff_lzw": (_i, [C.POINTER(TiffLzwItem), _i, _p, _i64, _p, _p, _p, _i64, _p]),
    "vx_tiff_unpredict_workspace_bytes": (_i64, [_i]),
    "vx_tiff_unpredict": (_i, [C.POINTER(TiffUnpredictItem), _i, _p, _p, _i64, _p]),
    "vx_tiff_predict_workspace_bytes": (_i64, [_i]),
    "vx_tiff_predict": (_i, [C.POINTER(TiffUnpredictItem), _i, _p, _p, _i64, _p]),
    "vx_tiff_lzw_bound": (_i64, [_i64]),
    "vx_tiff_lzw_encode_workspace_bytes": (_i64, [_i]),
    "vx_tiff_lzw_encode": (_i, [C.POINTER(TiffLzwItem), _i, _p, _i64, _p, _p, _p, _i64, _p]),
    "vx_tiff_lzw_pack_workspace_bytes": (_i64, [_i]),
    "vx_tiff_lzw_pack": (_i, [C.POINTER(TiffLzwItem), _i, _p, _i64, _p, _p, _i64, _p, _p, _i64, _p]),
}

_lib = None


class VxError(RuntimeError):
    pass


def load():
    """Load libvalues_amd.so (once).  import torch first: torch ships the HIP runtime
    (libamdhip64.so.7) this library resolves against, so both share one runtime instance."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VxError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C values_amd/csrc`). values_amd has no CPU fallback.")
    import torch  # noqa: F401  (loads the HIP runtime)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("VX_LIB_PATH") and not hasattr(lib, name):
            continue  # an A/B build of an older revision lacks the newer entry points
        fn = getattr(lib, name)  # AttributeError if the symbol is absent
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def get_config() -> "Config":
    c = Config()
    check(load().vx_get_config(C.byref(c)), "vx_get_config")
    return c


class config:
    """`with _lib.config(conv_fp32=1): ...` -- run a block under a changed vx_config (tests and A/B tools; the library
    reads its VX_* environment variables only once, at first use).  Restores the previous configuration on exit."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.saved = get_config()
        c = get_config()
        for k, v in self.fields.items():
            if not hasattr(c, k):
                raise AttributeError(f"vx_config has no field {k!r}")
            setattr(c, k, int(v))
        check(load().vx_set_config(C.byref(c)), "vx_set_config")
        return c

    def __exit__(self, *exc):
        check(load().vx_set_config(C.byref(self.saved)), "vx_set_config")
        return False


def pack_mode():
    """The configuration fields that select the kernel family and with it the PACKED WEIGHT LAYOUT (conv_config() and
    s16_config() in conv3d_route.h, conv2d_family() in conv2d_route.h).  Models key their packed-weight
    cache on it, and every launch carries the family its weights were packed for (w_family): the library refuses a
    mismatch."""
    c = get_config()
    return (c.conv_fp32, c.c2s_no_oct)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().vx_last_error_string()
        raise VxError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise VxError("values_amd needs a ROCm device (torch.cuda.is_available() is False); there is no CPU fallback")


def zeros(shape, dtype=None, device=None):
    """torch.empty + vx_zero on the current stream: a zero tensor without an ATen fill kernel (the persistent zero-padded
    buffers of the 2D walk are created through this, once per geometry)"""
    import torch
    require_gpu()
    t = torch.empty(shape, dtype=dtype or torch.float32, device=device)
    check(load().vx_zero(ptr(t), t.numel() * t.element_size(), stream_ptr()), "vx_zero")
    return t


_ws = {}


def workspace(dev, need):
    """the device's shared workspace for the batched entry points: a uint8 tensor of at least `need` bytes (64 KiB at the
    least) that only ever grows.  One buffer serves aggregation, evalmetrics and thresholds alike, which assumes what the
    per-module caches it replaces assumed: the callers of a device issue their calls from one thread onto one stream, so
    a call's kernels are ordered before the next call's on that stream.  Work on several streams or threads needs a
    workspace of its own per stream (the C entry points take any caller-owned buffer)."""
    import torch
    key = str(dev)
    if key not in _ws or _ws[key].numel() < need:
        _ws[key] = torch.empty(max(int(need), 1 << 16), dtype=torch.uint8, device=dev)
    return _ws[key]


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dense_block(t):
    """`t` itself when its elements fill one block of memory without gaps or overlap -- a contiguous tensor or a permuted
    view of one, such as the [x, y, z] views the readers return: data_ptr() is then the block's first element, and what an
    element-wise or order-free kernel computes does not depend on the order.  Anything else: a contiguous copy."""
    if t.is_contiguous():
        return t
    expect = 1
    for size, stride in sorted(((n, s) for n, s in zip(t.shape, t.stride()) if n != 1), key=lambda d: d[1]):
        if stride != expect:
            return t.contiguous()
        expect *= size
    return t


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())
