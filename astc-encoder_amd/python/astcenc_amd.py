# SPDX-License-Identifier: Apache-2.0
"""ctypes binding of the astcenc C ABI (include/astcenc.h + include/astcenc_amd.h).

LIB_PRODUCT is astc-encoder_amd/libastcenc_amd.so (HIP kernels, gfx950).  Library(path) binds any shared
object with the astcenc ABI, which is how the tests drive the checker libraries (their paths live in
oracle/oracle_libs.py, not here) through the very same calls: compress with A, compress with B, compare bytes.

Names mirror the C API (ref: Source/astcenc.h); see include/astcenc.h for field meaning.
"""
import ctypes as C
import os

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
LIB_PRODUCT = os.environ.get("ASTCENC_AMD_LIB", os.path.join(REPO, "astc-encoder_amd", "libastcenc_amd.so"))

# enum astcenc_error
(SUCCESS, ERR_OUT_OF_MEM, ERR_BAD_CPU_FLOAT, ERR_BAD_PARAM, ERR_BAD_BLOCK_SIZE, ERR_BAD_PROFILE,
 ERR_BAD_QUALITY, ERR_BAD_SWIZZLE, ERR_BAD_FLAGS, ERR_BAD_CONTEXT, ERR_NOT_IMPLEMENTED,
 ERR_BAD_DECODE_MODE) = range(12)
# enum astcenc_profile
PRF_LDR_SRGB, PRF_LDR, PRF_HDR_RGB_LDR_A, PRF_HDR = range(4)
# presets
PRE_FASTEST, PRE_FAST, PRE_MEDIUM, PRE_THOROUGH, PRE_VERYTHOROUGH, PRE_EXHAUSTIVE = 0.0, 10.0, 60.0, 98.0, 99.0, 100.0
# enum astcenc_swz
SWZ_R, SWZ_G, SWZ_B, SWZ_A, SWZ_0, SWZ_1, SWZ_Z = range(7)
# enum astcenc_type
TYPE_U8, TYPE_F16, TYPE_F32 = range(3)
# flags
FLG_MAP_NORMAL = 1 << 0
FLG_USE_DECODE_UNORM8 = 1 << 1
FLG_USE_ALPHA_WEIGHT = 1 << 2
FLG_USE_PERCEPTUAL = 1 << 3
FLG_DECOMPRESS_ONLY = 1 << 4
FLG_SELF_DECOMPRESS_ONLY = 1 << 5
FLG_MAP_RGBM = 1 << 6

PROGRESS_CB = C.CFUNCTYPE(None, C.c_float)


class Config(C.Structure):
    """struct astcenc_config (ref: astcenc.h:427)."""
    _fields_ = [
        ("profile", C.c_int), ("flags", C.c_uint),
        ("block_x", C.c_uint), ("block_y", C.c_uint), ("block_z", C.c_uint),
        ("cw_r_weight", C.c_float), ("cw_g_weight", C.c_float), ("cw_b_weight", C.c_float), ("cw_a_weight", C.c_float),
        ("a_scale_radius", C.c_uint), ("rgbm_m_scale", C.c_float),
        ("tune_partition_count_limit", C.c_uint),
        ("tune_2partition_index_limit", C.c_uint), ("tune_3partition_index_limit", C.c_uint), ("tune_4partition_index_limit", C.c_uint),
        ("tune_block_mode_limit", C.c_uint), ("tune_refinement_limit", C.c_uint), ("tune_candidate_limit", C.c_uint),
        ("tune_2partitioning_candidate_limit", C.c_uint), ("tune_3partitioning_candidate_limit", C.c_uint),
        ("tune_4partitioning_candidate_limit", C.c_uint),
        ("tune_db_limit", C.c_float), ("tune_mse_overshoot", C.c_float),
        ("tune_2partition_early_out_limit_factor", C.c_float), ("tune_3partition_early_out_limit_factor", C.c_float),
        ("tune_2plane_early_out_limit_correlation", C.c_float), ("tune_search_mode0_enable", C.c_float),
        ("progress_callback", PROGRESS_CB),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "progress_callback"}


class Image(C.Structure):
    """struct astcenc_image (ref: astcenc.h:613)."""
    _fields_ = [("dim_x", C.c_uint), ("dim_y", C.c_uint), ("dim_z", C.c_uint), ("data_type", C.c_int),
                ("data", C.POINTER(C.c_void_p))]


class Swizzle(C.Structure):
    """struct astcenc_swizzle (ref: astcenc.h:294)."""
    _fields_ = [("r", C.c_int), ("g", C.c_int), ("b", C.c_int), ("a", C.c_int)]


class BlockInfo(C.Structure):
    """struct astcenc_block_info (ref: astcenc.h:637-704)."""
    _fields_ = [("profile", C.c_int), ("block_x", C.c_uint), ("block_y", C.c_uint), ("block_z", C.c_uint), ("texel_count", C.c_uint),
                ("is_error_block", C.c_bool), ("is_constant_block", C.c_bool), ("is_hdr_block", C.c_bool), ("is_dual_plane_block", C.c_bool),
                ("partition_count", C.c_uint), ("partition_index", C.c_uint), ("dual_plane_component", C.c_uint),
                ("color_endpoint_modes", C.c_uint * 4), ("color_level_count", C.c_uint), ("weight_level_count", C.c_uint),
                ("weight_x", C.c_uint), ("weight_y", C.c_uint), ("weight_z", C.c_uint),
                ("color_endpoints", ((C.c_float * 4) * 2) * 4), ("weight_values_plane1", C.c_float * 216),
                ("weight_values_plane2", C.c_float * 216), ("partition_assignment", C.c_uint8 * 216)]


SWZ_RGBA = (SWZ_R, SWZ_G, SWZ_B, SWZ_A)

EXPORTS = ["astcenc_config_init", "astcenc_context_alloc", "astcenc_compress_image", "astcenc_compress_reset",
           "astcenc_compress_cancel", "astcenc_decompress_image", "astcenc_decompress_reset",
           "astcenc_context_free", "astcenc_get_block_info", "astcenc_get_error_string"]
EXPORTS_AMD = ["astcenc_amd_compress_image_device", "astcenc_amd_compress_volume_device", "astcenc_amd_decompress_image_device",
               "astcenc_amd_compare_images_device", "astcenc_amd_backend_name", "astcenc_amd_context_device_count",
               "astcenc_amd_context_set_option", "astcenc_amd_compare_images_hdr_device", "astcenc_amd_context_kernel_name",
               "astcenc_amd_set_log_callback", "astcenc_amd_context_specialize", "astcenc_amd_compress_images_device",
               "astcenc_amd_decompress_images_device", "astcenc_amd_mip_chain_layout", "astcenc_amd_generate_mip_chain_device",
               "astcenc_amd_compress_mip_chain_device", "astcenc_amd_mip_chain_volume_layout",
               "astcenc_amd_generate_mip_chain_volume_device", "astcenc_amd_compress_mip_chain_volume_device",
               "astcenc_amd_generate_mip_chain_ex_device", "astcenc_amd_compress_mip_chain_ex_device",
               "astcenc_amd_generate_mip_chain_filtered_device", "astcenc_amd_compress_mip_chain_filtered_device",
               "astcenc_amd_generate_mip_chain_weighted_device", "astcenc_amd_compress_mip_chain_weighted_device",
               "astcenc_amd_resize_image_device", "astcenc_amd_resize_dims", "astcenc_amd_compare_blocks_device",
               "astcenc_amd_compare_blocks_hdr_device", "astcenc_amd_compare_image_set_device",
               "astcenc_amd_compress_block_list_device", "astcenc_amd_select_blocks_device",
               "astcenc_amd_compress_image_adaptive_device", "astcenc_amd_select_blocks_set_device",
               "astcenc_amd_compress_block_list_set_device", "astcenc_amd_compress_images_adaptive_device",
               "astcenc_amd_decompress_regions_device", "astcenc_amd_decompress_tensors_device",
               "astcenc_amd_decompress_scaled_tensors_device", "astcenc_amd_sample_tensors_device",
               "astcenc_amd_sample_lod_tensors_device", "astcenc_amd_sample_cube_tensors_device",
               "astcenc_amd_sample_volume_tensors_device", "astcenc_amd_sample_lod_grad_device",
               "astcenc_amd_sample_volume_grad_device"]
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_PLANAR, TENSOR_INTERLEAVED = 0, 1
TENSOR_FLIP_X, TENSOR_FLIP_Y = 0x1, 0x2
WINDOW_BILINEAR, WINDOW_BOX = 0, 1
SAMPLE_NEAREST, SAMPLE_BILINEAR = 0, 1
MIP_NEAREST, MIP_LINEAR = 0, 1
ADDRESS_CLAMP, ADDRESS_REPEAT, ADDRESS_MIRROR, ADDRESS_BORDER = 0, 1, 2, 3
NO_BLOCK_BUDGET = 0xFFFFFFFF
OPT_PER_SLICE_FAST_LOAD = 1
MAX_MIP_LEVELS = 32
MIP_ARRAY, MIP_VOLUME = 0, 1
MIP_NORMALIZE, MIP_ALPHA_COVERAGE = 0x1, 0x2
MIP_FILTER_BOX, MIP_FILTER_MITCHELL, MIP_FILTER_LANCZOS3, MIP_FILTER_KAISER = 0, 1, 2, 3
MIP_EDGE_CLAMP, MIP_EDGE_WRAP, MIP_EDGE_CUBE = 0, 1, 2
MIP_WEIGHT_NONE, MIP_WEIGHT_ALPHA = 0, 1
POW2_NONE, POW2_NEAREST, POW2_NEXT, POW2_PREVIOUS = 0, 1, 2, 3


class MipChainLayout(C.Structure):
    """struct astcenc_amd_mip_chain_layout (include/astcenc_amd.h)."""
    _fields_ = [("level_count", C.c_uint), ("dim_x", C.c_uint * MAX_MIP_LEVELS), ("dim_y", C.c_uint * MAX_MIP_LEVELS),
                ("texels_offset", C.c_size_t * MAX_MIP_LEVELS), ("blocks_offset", C.c_size_t * MAX_MIP_LEVELS),
                ("texels_len", C.c_size_t), ("blocks_len", C.c_size_t)]


class MipChainVolumeLayout(C.Structure):
    """struct astcenc_amd_mip_chain_volume_layout (include/astcenc_amd.h)."""
    _fields_ = [("level_count", C.c_uint), ("dim_x", C.c_uint * MAX_MIP_LEVELS), ("dim_y", C.c_uint * MAX_MIP_LEVELS),
                ("dim_z", C.c_uint * MAX_MIP_LEVELS), ("texels_offset", C.c_size_t * MAX_MIP_LEVELS),
                ("blocks_offset", C.c_size_t * MAX_MIP_LEVELS), ("texels_len", C.c_size_t), ("blocks_len", C.c_size_t)]


class MipOptions(C.Structure):
    """struct astcenc_amd_mip_options (include/astcenc_amd.h): flags = MIP_NORMALIZE | MIP_ALPHA_COVERAGE, alpha_cutoff."""
    _fields_ = [("flags", C.c_uint), ("alpha_cutoff", C.c_float)]


class MipFilter(C.Structure):
    """struct astcenc_amd_mip_filter (include/astcenc_amd.h): kind = MIP_FILTER_*, edge = MIP_EDGE_*."""
    _fields_ = [("kind", C.c_int), ("edge", C.c_int)]


class MipWeighting(C.Structure):
    """struct astcenc_amd_mip_weighting (include/astcenc_amd.h): weight = MIP_WEIGHT_*."""
    _fields_ = [("weight", C.c_int)]


class Resize(C.Structure):
    """struct astcenc_amd_resize (include/astcenc_amd.h): the destination size, the filter and the weighting."""
    _fields_ = [("dim_x", C.c_uint), ("dim_y", C.c_uint), ("dim_z", C.c_uint), ("filter", MipFilter), ("weighting", MipWeighting)]


class ImageSetEntry(C.Structure):
    """struct astcenc_amd_image_set_entry (include/astcenc_amd.h)."""
    _fields_ = [("image", C.c_void_p), ("blocks", C.c_void_p), ("blocks_len", C.c_size_t),
                ("dim_x", C.c_uint), ("dim_y", C.c_uint), ("dim_z", C.c_uint), ("data_type", C.c_int), ("swizzle", Swizzle)]


def image_set_entry(image, blocks, swizzle=SWZ_RGBA, blocks_len=None):
    """ImageSetEntry of two device tensors: `image` [H, W, 4] or [D, H, W, 4] of uint8 / float16 / float32 (contiguous) and
    `blocks`, uint8 (blocks_len: its size in bytes unless given)."""
    import torch
    types = {torch.uint8: TYPE_U8, torch.float16: TYPE_F16, torch.float32: TYPE_F32}
    assert image.is_contiguous() and blocks.is_contiguous() and image.dim() in (3, 4) and image.shape[-1] == 4
    d = image.shape[0] if image.dim() == 4 else 1
    h, w = image.shape[-3], image.shape[-2]
    return ImageSetEntry(image.data_ptr(), blocks.data_ptr(), blocks.numel() * blocks.element_size() if blocks_len is None else blocks_len,
                         w, h, d, types[image.dtype], Swizzle(*swizzle))


def compressed_entry(blocks, dims, data_type, swizzle=SWZ_RGBA, blocks_len=None):
    """ImageSetEntry of a compressed image alone (astcenc_amd_decompress_regions_device ignores `image`): `blocks` a uint8
    device tensor, dims (dim_x, dim_y[, dim_z]), data_type the TYPE_* its windows are decoded to."""
    assert blocks.is_contiguous()
    dz = dims[2] if len(dims) > 2 else 1
    return ImageSetEntry(None, blocks.data_ptr(), blocks.numel() * blocks.element_size() if blocks_len is None else blocks_len,
                         dims[0], dims[1], dz, data_type, Swizzle(*swizzle))


class DecodeRegion(C.Structure):
    """struct astcenc_amd_decode_region (include/astcenc_amd.h)."""
    _fields_ = [("entry", C.c_uint), ("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint),
                ("size_x", C.c_uint), ("size_y", C.c_uint), ("size_z", C.c_uint),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("slice_pitch", C.c_size_t)]


def decode_region(entry, origin, size, out):
    """DecodeRegion of window `size` = (size_x, size_y, size_z) at `origin` = (x, y, z) of entry `entry`.  `out`: a device
    tensor view [size_y, size_x, 4] or [size_z, size_y, size_x, 4] whose pitches are taken from its strides (the texels of a row
    must be contiguous: strides (..., 4, 1)), or an explicit (ptr, row_pitch, slice_pitch) in bytes (0 = tightly packed)."""
    if isinstance(out, tuple):
        ptr, row_pitch, slice_pitch = out
    else:
        assert out.dim() in (3, 4) and out.shape[-1] == 4, "out is [size_y, size_x, 4] or [size_z, size_y, size_x, 4]"
        assert tuple(out.shape[-3:-1]) == (size[1], size[0]) and (out.shape[0] if out.dim() == 4 else 1) == size[2], "out does not have the window's shape"
        st = out.stride()
        if st[-1] != 1 or st[-2] != 4:
            raise ValueError("the texels of a row of `out` are not contiguous (strides %r)" % (tuple(st),))
        item = out.element_size()
        ptr, row_pitch = out.data_ptr(), st[-3] * item
        slice_pitch = st[0] * item if out.dim() == 4 else 0
    return DecodeRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], size[2], ptr, row_pitch, slice_pitch)


class TensorFormat(C.Structure):
    """struct astcenc_amd_tensor_format (include/astcenc_amd.h)."""
    _fields_ = [("type", C.c_int), ("layout", C.c_int), ("channels", C.c_uint), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


def tensor_format(type, layout, channels, scale=(1.0,) * 4, bias=(0.0,) * 4):
    """TensorFormat from TENSOR_* constants and per-channel sequences (shorter ones are padded with scale 1, bias 0)."""
    scale, bias = list(scale) + [1.0] * (4 - len(scale)), list(bias) + [0.0] * (4 - len(bias))
    return TensorFormat(type, layout, channels, (C.c_float * 4)(*scale[:4]), (C.c_float * 4)(*bias[:4]))


class TensorRegion(C.Structure):
    """struct astcenc_amd_tensor_region (include/astcenc_amd.h)."""
    _fields_ = [("entry", C.c_uint), ("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint),
                ("size_x", C.c_uint), ("size_y", C.c_uint), ("size_z", C.c_uint), ("flags", C.c_uint),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("slice_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def tensor_region(entry, origin, size, out_view, flip_x=False, flip_y=False, layout=TENSOR_PLANAR):
    """TensorRegion of window `size` = (size_x, size_y, size_z) at `origin` = (x, y, z) of entry `entry`, written into the torch
    view `out_view`: [C, H, W] or [C, D, H, W] for TENSOR_PLANAR, [H, W, C] or [D, H, W, C] for TENSOR_INTERLEAVED, with H, W, D
    the window's size_y, size_x, size_z and C the format's channels.  Pointer and pitches (in elements) come from the view's
    strides; ValueError for strides the layout cannot express: columns that are not `1` (planar) or `C` (interleaved) elements
    apart, interleaved channels that are not adjacent, a negative stride.  Or an explicit (ptr, row_pitch, slice_pitch,
    plane_pitch) in elements (0 = tightly packed)."""
    flags = (TENSOR_FLIP_X if flip_x else 0) | (TENSOR_FLIP_Y if flip_y else 0)
    if isinstance(out_view, tuple):
        ptr, row_pitch, slice_pitch, plane_pitch = out_view
        return TensorRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], size[2], flags, ptr, row_pitch, slice_pitch, plane_pitch)
    shape, st = tuple(out_view.shape), tuple(out_view.stride())
    if out_view.dim() not in (3, 4):
        raise ValueError("out_view has %d dimensions: [C, H, W], [C, D, H, W], [H, W, C] or [D, H, W, C]" % out_view.dim())
    if any(v < 0 for v in st):
        raise ValueError("out_view has a negative stride %r" % (st,))
    if layout == TENSOR_PLANAR:
        depth = shape[1] if len(shape) == 4 else 1
        if (shape[-1], shape[-2], depth) != tuple(size):
            raise ValueError("out_view %r does not have the window's shape %r" % (shape, tuple(size)))
        if st[-1] != 1 and shape[-1] > 1:
            raise ValueError("the columns of a planar view must be adjacent elements (strides %r)" % (st,))
        row_pitch, slice_pitch, plane_pitch = st[-2], (st[1] if len(shape) == 4 else 0), st[0]
    else:
        depth = shape[0] if len(shape) == 4 else 1
        if (shape[-2], shape[-3], depth) != tuple(size):
            raise ValueError("out_view %r does not have the window's shape %r" % (shape, tuple(size)))
        if (st[-1] != 1 and shape[-1] > 1) or (st[-2] != shape[-1] and shape[-2] > 1):
            raise ValueError("the channels of an interleaved view must be adjacent and its columns C elements apart (strides %r)" % (st,))
        row_pitch, slice_pitch, plane_pitch = st[-3], (st[0] if len(shape) == 4 else 0), 0
    return TensorRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], size[2], flags, out_view.data_ptr(), row_pitch, slice_pitch, plane_pitch)


class ScaledRegion(C.Structure):
    """struct astcenc_amd_scaled_region (include/astcenc_amd.h)."""
    _fields_ = [("entry", C.c_uint), ("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint),
                ("size_x", C.c_uint), ("size_y", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint), ("flags", C.c_uint),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def scaled_region(entry, origin, size, out_view, flip_x=False, flip_y=False, layout=TENSOR_PLANAR, type=None):
    """ScaledRegion of window `size` = (size_x, size_y) at `origin` = (x, y, z) of entry `entry`, resampled into the torch view
    `out_view`: [C, H, W] for TENSOR_PLANAR, [H, W, C] for TENSOR_INTERLEAVED -- out_x, out_y are its W and H, pointer and pitches
    (in elements) come from its strides.  ValueError for a view the layouts cannot express: not three dimensions, columns that
    are not `1` (planar) or `C` (interleaved) elements apart, interleaved channels that are not adjacent, a negative stride, a
    zero stride along an axis longer than one (an expanded view: its rows or planes alias each other, and a zero pitch means
    `tightly packed` to the call), a size outside 1 .. 65535; with `type` (the format's TENSOR_*), also for a view of another
    dtype.  Or an explicit (ptr, out_x, out_y, row_pitch, plane_pitch) in elements (0 = tightly packed)."""
    flags = (TENSOR_FLIP_X if flip_x else 0) | (TENSOR_FLIP_Y if flip_y else 0)
    if isinstance(out_view, tuple):
        ptr, out_x, out_y, row_pitch, plane_pitch = out_view
        return ScaledRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], out_x, out_y, flags, ptr, row_pitch, plane_pitch)
    shape, st = tuple(out_view.shape), tuple(out_view.stride())
    if out_view.dim() != 3:
        raise ValueError("out_view has %d dimensions: [C, H, W] or [H, W, C]" % out_view.dim())
    if any(v < 0 for v in st):
        raise ValueError("out_view has a negative stride %r" % (st,))
    if any(v == 0 and n > 1 for v, n in zip(st, shape)):
        raise ValueError("out_view has a zero stride along an axis longer than one (shape %r, strides %r): its elements alias" % (shape, st))
    if type is not None:
        import torch
        want = {TENSOR_F32: torch.float32, TENSOR_F16: torch.float16, TENSOR_BF16: torch.bfloat16}.get(type)
        if out_view.dtype != want:
            raise ValueError("out_view is %s, the format's type %r is %s" % (out_view.dtype, type, want))
    if layout == TENSOR_PLANAR:
        out_x, out_y = shape[2], shape[1]
        if st[2] != 1 and out_x > 1:
            raise ValueError("the columns of a planar view must be adjacent elements (strides %r)" % (st,))
        row_pitch, plane_pitch = st[1], st[0]
    else:
        out_x, out_y = shape[1], shape[0]
        if (st[2] != 1 and shape[2] > 1) or (st[1] != shape[2] and out_x > 1):
            raise ValueError("the channels of an interleaved view must be adjacent and its columns C elements apart (strides %r)" % (st,))
        row_pitch, plane_pitch = st[0], 0
    if not (1 <= out_x <= 65535 and 1 <= out_y <= 65535 and 1 <= size[0] <= 65535 and 1 <= size[1] <= 65535):
        raise ValueError("window %r to %r: every size is 1 .. 65535" % (tuple(size), (out_x, out_y)))
    # (the stride of an axis of length one says nothing: the tight pitch)
    if out_y == 1:
        row_pitch = 0
    if layout == TENSOR_PLANAR and shape[0] == 1:
        plane_pitch = 0
    return ScaledRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], out_x, out_y, flags, out_view.data_ptr(), row_pitch, plane_pitch)


class Sampler(C.Structure):
    """struct astcenc_amd_sampler (include/astcenc_amd.h): SAMPLE_* filter, ADDRESS_* mode per axis."""
    _fields_ = [("filter", C.c_int), ("address_x", C.c_int), ("address_y", C.c_int)]


class SampleGrid(C.Structure):
    """struct astcenc_amd_sample_grid (include/astcenc_amd.h)."""
    _fields_ = [("entry", C.c_uint), ("z", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("coords", C.c_void_p), ("coord_row_pitch", C.c_size_t),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def sample_grid(entry, z, coords, out_view, layout=TENSOR_PLANAR, type=None):
    """SampleGrid of slice `z` of entry `entry`: `coords` is a float32 torch tensor [H, W, 2] of (x, y) pairs in texel units,
    `out_view` the torch view [C, H, W] for TENSOR_PLANAR or [H, W, C] for TENSOR_INTERLEAVED the points are written to;
    pointers and pitches (in floats / elements) come from the strides.  ValueError for what the call cannot express: coordinates
    that are not float32, not [H, W, 2], whose pairs are not adjacent or not two floats apart, whose rows are an odd number of
    floats apart or which do not start on 8 bytes; an output of another H, W; the views scaled_region rejects (not three
    dimensions, columns not `1` / `C` elements apart, channels not adjacent, negative or aliasing zero strides, a size outside
    1 .. 65535, with `type` another dtype).  Or explicit tuples: coords = (ptr, out_x, out_y, coord_row_pitch) and out_view =
    (ptr, row_pitch, plane_pitch)."""
    if isinstance(coords, tuple):
        cptr, out_x, out_y, coord_row_pitch = coords
        optr, row_pitch, plane_pitch = out_view
        return SampleGrid(entry, z, out_x, out_y, cptr, coord_row_pitch, optr, row_pitch, plane_pitch)
    import torch
    if coords.dtype != torch.float32:
        raise ValueError("coords is %s: float32 pairs" % coords.dtype)
    cshape, cst = tuple(coords.shape), tuple(coords.stride())
    if coords.dim() != 3 or cshape[2] != 2:
        raise ValueError("coords has shape %r: [H, W, 2]" % (cshape,))
    if cst[2] != 1 or (cst[1] != 2 and cshape[1] > 1) or cst[0] < 0 or (cst[0] == 0 and cshape[0] > 1) or cst[0] % 2 != 0:
        raise ValueError("the pairs of coords must be adjacent floats, two floats apart, its rows an even number of floats apart (strides %r)" % (cst,))
    if coords.data_ptr() % 8 != 0:
        raise ValueError("coords does not start on 8 bytes")
    # (the output's checks are scaled_region's: a window of 1 x 1 stands in for the one this call does not have)
    r = scaled_region(entry, (0, 0, z), (1, 1), out_view, layout=layout, type=type)
    if (r.out_x, r.out_y) != (cshape[1], cshape[0]):
        raise ValueError("out_view is %u x %u points, coords %u x %u" % (r.out_x, r.out_y, cshape[1], cshape[0]))
    coord_row_pitch = cst[0] if cshape[0] > 1 else 0
    if coord_row_pitch != 0 and coord_row_pitch < 2 * cshape[1]:
        raise ValueError("the rows of coords overlap (strides %r)" % (cst,))
    return SampleGrid(entry, z, r.out_x, r.out_y, coords.data_ptr(), coord_row_pitch, r.out, r.row_pitch, r.plane_pitch)


class LodSampler(C.Structure):
    """struct astcenc_amd_lod_sampler (include/astcenc_amd.h): SAMPLE_* filter within a level, ADDRESS_* mode per axis, MIP_NEAREST /
    MIP_LINEAR between levels."""
    _fields_ = [("filter", C.c_int), ("address_x", C.c_int), ("address_y", C.c_int), ("mip_filter", C.c_int)]


class LodGrid(C.Structure):
    """struct astcenc_amd_lod_grid (include/astcenc_amd.h)."""
    _fields_ = [("first_entry", C.c_uint), ("level_count", C.c_uint), ("z", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("coords", C.c_void_p), ("coord_row_pitch", C.c_size_t), ("lod", C.c_void_p), ("lod_row_pitch", C.c_size_t), ("lod_bias", C.c_float),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def _check_chain(level_count, lod_bias):
    """What lod_grid, cube_grid and volume_grid reject of a chain's length and of the bias."""
    import math
    if not 1 <= level_count <= MAX_MIP_LEVELS:
        raise ValueError("level_count %r: a chain has 1 .. %d levels" % (level_count, MAX_MIP_LEVELS))
    if not math.isfinite(lod_bias):
        raise ValueError("lod_bias %r is not finite" % (lod_bias,))


def _lod_buffer(lod, out_x, out_y, device, other):
    """(pointer, lod_row_pitch) of a float32 torch tensor [out_y, out_x] of levels of detail, or (None, 0) for None; ValueError
    for what lod_grid's comment lists.  `device` is that of the points' tensor, which `other` names."""
    if lod is None:
        return None, 0
    import torch
    if lod.dtype != torch.float32:
        raise ValueError("lod is %s: float32" % lod.dtype)
    lshape, lst = tuple(lod.shape), tuple(lod.stride())
    if lod.dim() != 2 or lshape != (out_y, out_x):
        raise ValueError("lod has shape %r: [H, W] = [%u, %u]" % (lshape, out_y, out_x))
    if (lst[1] != 1 and lshape[1] > 1) or lst[0] < 0 or (lst[0] == 0 and lshape[0] > 1):
        raise ValueError("the columns of lod must be adjacent floats and its rows apart (strides %r)" % (lst,))
    if lod.device != device:
        raise ValueError("lod is on %s, %s on %s" % (lod.device, other, device))
    lod_row_pitch = lst[0] if lshape[0] > 1 else 0
    if lod_row_pitch != 0 and lod_row_pitch < lshape[1]:
        raise ValueError("the rows of lod overlap (strides %r)" % (lst,))
    return lod.data_ptr(), lod_row_pitch


def lod_grid(first_entry, level_count, z, coords, lod, out_view, lod_bias=0.0, layout=TENSOR_PLANAR, type=None):
    """LodGrid of slice `z` of the chain entries[first_entry : first_entry + level_count]: `coords` is a float32 torch tensor
    [H, W, 2] of NORMALISED (u, v) pairs, `lod` a float32 torch tensor [H, W] of levels of detail or None (0 everywhere), `out_view`
    the torch view [C, H, W] for TENSOR_PLANAR or [H, W, C] for TENSOR_INTERLEAVED the points are written to; pointers and pitches
    come from the strides.  ValueError for what the call cannot express: everything sample_grid rejects of `coords` and `out_view`;
    a level_count outside 1 .. 32; a lod_bias that is not finite; a `lod` that is not float32, not [H, W] with the H, W of `coords`,
    whose columns are not adjacent floats, whose rows overlap or alias or have a negative stride, or which lives on another device
    than `coords`.  Or explicit tuples: coords = (ptr, out_x, out_y, coord_row_pitch), lod = (ptr, lod_row_pitch) or None, out_view =
    (ptr, row_pitch, plane_pitch)."""
    _check_chain(level_count, lod_bias)
    if isinstance(coords, tuple):
        g = sample_grid(first_entry, z, coords, out_view)
        lptr, lod_row_pitch = lod if lod is not None else (None, 0)
    else:
        g = sample_grid(first_entry, z, coords, out_view, layout=layout, type=type)
        lptr, lod_row_pitch = _lod_buffer(lod, g.out_x, g.out_y, coords.device, "coords")
    return LodGrid(first_entry, level_count, z, g.out_x, g.out_y, g.coords, g.coord_row_pitch, lptr, lod_row_pitch, lod_bias, g.out, g.row_pitch, g.plane_pitch)


class LodGradGrid(C.Structure):
    """struct astcenc_amd_lod_grad_grid (include/astcenc_amd.h)."""
    _fields_ = [("first_entry", C.c_uint), ("level_count", C.c_uint), ("z", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("coords", C.c_void_p), ("coord_row_pitch", C.c_size_t), ("lod", C.c_void_p), ("lod_row_pitch", C.c_size_t), ("lod_bias", C.c_float),
                ("grad_out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t),
                ("grad_coords", C.c_void_p), ("grad_coord_row_pitch", C.c_size_t), ("grad_lod", C.c_void_p), ("grad_lod_row_pitch", C.c_size_t)]


def lod_grad_grid(first_entry, level_count, z, coords, lod, grad_out, grad_coords, grad_lod=None, lod_bias=0.0, layout=TENSOR_PLANAR, type=None):
    """LodGradGrid of the forward grid lod_grid(first_entry, level_count, z, coords, lod, <out>): `grad_out` is the torch view of the
    upstream gradient, of the forward output's shape and type ([C, H, W] or [H, W, C]); `grad_coords` a float32 torch tensor
    [H, W, 2] and `grad_lod` a float32 torch tensor [H, W] or None (not wanted), which are written.  ValueError for everything
    lod_grid rejects -- of `grad_out` what it rejects of the output, of `grad_coords` what it rejects of `coords`, of `grad_lod`
    what it rejects of `lod` -- and for a `grad_coords` of another H, W or on another device than `coords`.  Or explicit tuples:
    coords = (ptr, out_x, out_y, coord_row_pitch), lod = (ptr, lod_row_pitch) or None, grad_out = (ptr, row_pitch, plane_pitch),
    grad_coords = (ptr, grad_coord_row_pitch), grad_lod = (ptr, grad_lod_row_pitch) or None."""
    g = lod_grid(first_entry, level_count, z, coords, lod, grad_out, lod_bias=lod_bias, layout=layout, type=type)
    if isinstance(coords, tuple):
        gcptr, grad_coord_row_pitch = grad_coords
        glptr, grad_lod_row_pitch = grad_lod if grad_lod is not None else (None, 0)
    else:
        # (the pairs of gradients are laid out as pairs of coordinates are: sample_grid's checks, with a view that passes them as the output)
        w = sample_grid(first_entry, z, grad_coords, grad_out, layout=layout, type=type)
        if grad_coords.device != coords.device:
            raise ValueError("grad_coords is on %s, coords on %s" % (grad_coords.device, coords.device))
        gcptr, grad_coord_row_pitch = w.coords, w.coord_row_pitch
        glptr, grad_lod_row_pitch = _lod_buffer(grad_lod, g.out_x, g.out_y, coords.device, "coords")
    return LodGradGrid(first_entry, level_count, z, g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, lod_bias, g.out, g.row_pitch, g.plane_pitch,
                       gcptr, grad_coord_row_pitch, glptr, grad_lod_row_pitch)


def _triple_grid(first_entry, level_count, name, points, lod, out_view, lod_bias, layout, type):
    """What cube_grid and volume_grid share: the fields out_x .. plane_pitch of their grids from `points`, a float32 torch tensor
    [H, W, 3] named `name` in the errors -- adjacent triples, rows apart -- an output of the same H x W and a lod buffer; or from
    the explicit tuples.  ValueError as the two say."""
    _check_chain(level_count, lod_bias)
    if isinstance(points, tuple):
        pptr, out_x, out_y, point_row_pitch = points
        optr, row_pitch, plane_pitch = out_view
        lptr, lod_row_pitch = lod if lod is not None else (None, 0)
        return out_x, out_y, pptr, point_row_pitch, lptr, lod_row_pitch, lod_bias, optr, row_pitch, plane_pitch
    import torch
    if points.dtype != torch.float32:
        raise ValueError("%s is %s: float32 triples" % (name, points.dtype))
    shape, st = tuple(points.shape), tuple(points.stride())
    if points.dim() != 3 or shape[2] != 3:
        raise ValueError("%s has shape %r: [H, W, 3]" % (name, shape))
    if st[2] != 1 or (st[1] != 3 and shape[1] > 1) or st[0] < 0 or (st[0] == 0 and shape[0] > 1):
        raise ValueError("the triples of %s must be adjacent floats, three floats apart, its rows apart (strides %r)" % (name, st))
    point_row_pitch = st[0] if shape[0] > 1 else 0
    if point_row_pitch != 0 and point_row_pitch < 3 * shape[1]:
        raise ValueError("the rows of %s overlap (strides %r)" % (name, st))
    # (the output's checks are scaled_region's: a window of 1 x 1 stands in for the one this call does not have)
    r = scaled_region(first_entry, (0, 0, 0), (1, 1), out_view, layout=layout, type=type)
    if (r.out_x, r.out_y) != (shape[1], shape[0]):
        raise ValueError("out_view is %u x %u points, %s %u x %u" % (r.out_x, r.out_y, name, shape[1], shape[0]))
    lptr, lod_row_pitch = _lod_buffer(lod, r.out_x, r.out_y, points.device, name)
    return r.out_x, r.out_y, points.data_ptr(), point_row_pitch, lptr, lod_row_pitch, lod_bias, r.out, r.row_pitch, r.plane_pitch


class CubeSampler(C.Structure):
    """struct astcenc_amd_cube_sampler (include/astcenc_amd.h): SAMPLE_* filter within a level, MIP_NEAREST / MIP_LINEAR between
    levels."""
    _fields_ = [("filter", C.c_int), ("mip_filter", C.c_int)]


class CubeGrid(C.Structure):
    """struct astcenc_amd_cube_grid (include/astcenc_amd.h)."""
    _fields_ = [("first_entry", C.c_uint), ("level_count", C.c_uint), ("cube", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("dirs", C.c_void_p), ("dir_row_pitch", C.c_size_t), ("lod", C.c_void_p), ("lod_row_pitch", C.c_size_t), ("lod_bias", C.c_float),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def cube_grid(first_entry, level_count, cube, dirs, lod, out_view, lod_bias=0.0, layout=TENSOR_PLANAR, type=None):
    """CubeGrid of cube `cube` of the chain entries[first_entry : first_entry + level_count]: `dirs` is a float32 torch tensor
    [H, W, 3] of directions (dx, dy, dz), `lod` a float32 torch tensor [H, W] or None, `out_view` the torch view [C, H, W] for
    TENSOR_PLANAR or [H, W, C] for TENSOR_INTERLEAVED; pointers and pitches come from the strides.  ValueError for what the call
    cannot express: directions that are not float32, not [H, W, 3], whose triples are not adjacent or not three floats apart or
    whose rows overlap; everything lod_grid rejects of `lod`, `out_view`, level_count and lod_bias.  Or explicit tuples: dirs =
    (ptr, out_x, out_y, dir_row_pitch), lod = (ptr, lod_row_pitch) or None, out_view = (ptr, row_pitch, plane_pitch)."""
    return CubeGrid(first_entry, level_count, cube, *_triple_grid(first_entry, level_count, "dirs", dirs, lod, out_view, lod_bias, layout, type))


class VolumeSampler(C.Structure):
    """struct astcenc_amd_volume_sampler (include/astcenc_amd.h): SAMPLE_* filter within a level (SAMPLE_BILINEAR is linear on all
    three axes), ADDRESS_* mode per axis, MIP_NEAREST / MIP_LINEAR between levels."""
    _fields_ = [("filter", C.c_int), ("address_x", C.c_int), ("address_y", C.c_int), ("address_z", C.c_int), ("mip_filter", C.c_int)]


class VolumeGrid(C.Structure):
    """struct astcenc_amd_volume_grid (include/astcenc_amd.h)."""
    _fields_ = [("first_entry", C.c_uint), ("level_count", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("coords", C.c_void_p), ("coord_row_pitch", C.c_size_t), ("lod", C.c_void_p), ("lod_row_pitch", C.c_size_t), ("lod_bias", C.c_float),
                ("out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t)]


def volume_grid(first_entry, level_count, coords, lod, out_view, lod_bias=0.0, layout=TENSOR_PLANAR, type=None):
    """VolumeGrid of the chain entries[first_entry : first_entry + level_count]: `coords` is a float32 torch tensor [H, W, 3] of
    NORMALISED (u, v, w) triples -- [1, N, 3] is a list of ray-march samples -- `lod` a float32 torch tensor [H, W] or None,
    `out_view` the torch view [C, H, W] for TENSOR_PLANAR or [H, W, C] for TENSOR_INTERLEAVED; pointers and pitches come from the
    strides.  ValueError for what the call cannot express: coordinates that are not float32, not [H, W, 3], whose triples are not
    adjacent or not three floats apart or whose rows overlap; everything lod_grid rejects of `lod`, `out_view`, level_count and
    lod_bias.  Or explicit tuples: coords = (ptr, out_x, out_y, coord_row_pitch), lod = (ptr, lod_row_pitch) or None, out_view =
    (ptr, row_pitch, plane_pitch)."""
    return VolumeGrid(first_entry, level_count, *_triple_grid(first_entry, level_count, "coords", coords, lod, out_view, lod_bias, layout, type))


class VolumeGradGrid(C.Structure):
    """struct astcenc_amd_volume_grad_grid (include/astcenc_amd.h)."""
    _fields_ = [("first_entry", C.c_uint), ("level_count", C.c_uint), ("out_x", C.c_uint), ("out_y", C.c_uint),
                ("coords", C.c_void_p), ("coord_row_pitch", C.c_size_t), ("lod", C.c_void_p), ("lod_row_pitch", C.c_size_t), ("lod_bias", C.c_float),
                ("grad_out", C.c_void_p), ("row_pitch", C.c_size_t), ("plane_pitch", C.c_size_t),
                ("grad_coords", C.c_void_p), ("grad_coord_row_pitch", C.c_size_t), ("grad_lod", C.c_void_p), ("grad_lod_row_pitch", C.c_size_t)]


def volume_grad_grid(first_entry, level_count, coords, lod, grad_out, grad_coords, grad_lod=None, lod_bias=0.0, layout=TENSOR_PLANAR, type=None):
    """VolumeGradGrid of the forward grid volume_grid(first_entry, level_count, coords, lod, <out>): `grad_out` is the torch view of
    the upstream gradient, of the forward output's shape and type ([C, H, W] or [H, W, C]); `grad_coords` a float32 torch tensor
    [H, W, 3] and `grad_lod` a float32 torch tensor [H, W] or None (not wanted), which are written.  ValueError for everything
    volume_grid rejects -- of `grad_out` what it rejects of the output, of `grad_coords` what it rejects of `coords`, of `grad_lod`
    what it rejects of `lod` -- and for a `grad_coords` of another H, W or on another device than `coords`.  Or explicit tuples:
    coords = (ptr, out_x, out_y, coord_row_pitch), lod = (ptr, lod_row_pitch) or None, grad_out = (ptr, row_pitch, plane_pitch),
    grad_coords = (ptr, grad_coord_row_pitch), grad_lod = (ptr, grad_lod_row_pitch) or None."""
    g = _triple_grid(first_entry, level_count, "coords", coords, lod, grad_out, lod_bias, layout, type)
    if isinstance(coords, tuple):
        gcptr, grad_coord_row_pitch = grad_coords
        glptr, grad_lod_row_pitch = grad_lod if grad_lod is not None else (None, 0)
    else:
        # (the triples of gradients are laid out as the triples of coordinates are: the same checks, grad_lod in the place of lod)
        w = _triple_grid(first_entry, level_count, "grad_coords", grad_coords, grad_lod, grad_out, lod_bias, layout, type)
        if grad_coords.device != coords.device:
            raise ValueError("grad_coords is on %s, coords on %s" % (grad_coords.device, coords.device))
        gcptr, grad_coord_row_pitch, glptr, grad_lod_row_pitch = w[2], w[3], w[4], w[5]
    return VolumeGradGrid(first_entry, level_count, *(g + (gcptr, grad_coord_row_pitch, glptr, grad_lod_row_pitch)))


class ErrorSums(C.Structure):
    """struct astcenc_amd_error_sums (include/astcenc_amd.h)."""
    _fields_ = [("squared_error", C.c_double * 4), ("alpha_scaled_squared_error", C.c_double * 4),
                ("rgb_peak", C.c_double), ("texels", C.c_double)]

    def psnr(self, channels=4, alpha_scaled=False):
        """PSNR over the first `channels` channels as the reference CLI reports it (999 dB when identical)."""
        src = self.alpha_scaled_squared_error if alpha_scaled else self.squared_error
        num = sum(src[k] for k in range(channels))
        return 999.0 if num == 0 else 10.0 * float(np.log10(self.texels * channels / num))


class HdrErrorSums(C.Structure):
    """struct astcenc_amd_hdr_error_sums (include/astcenc_amd.h)."""
    _fields_ = [("log2_squared_error", C.c_double * 4), ("mpsnr_squared_error", C.c_double * 4),
                ("fstop_lo", C.c_int), ("fstop_hi", C.c_int)]

    def mpsnr(self, texels):
        """mPSNR (RGB) as the reference CLI prints it (astcenccli_error_metrics.cpp:389-397)."""
        num = sum(self.mpsnr_squared_error[k] for k in range(3))
        stops = self.fstop_hi - self.fstop_lo + 1
        return 999.0 if num == 0 else 10.0 * float(np.log10(texels * 3.0 * stops * 255.0 * 255.0 / num))

    def log_rmse(self, texels):
        """LogRMSE (RGB) (astcenccli_error_metrics.cpp:402-403)."""
        return float(np.sqrt(sum(self.log2_squared_error[k] for k in range(3)) / texels))


class BlockError(C.Structure):
    """struct astcenc_amd_block_error (include/astcenc_amd.h): 32 bytes per block, raster block order."""
    _fields_ = [("squared_error", C.c_double * 4)]


class BlockCriterion(C.Structure):
    """struct astcenc_amd_block_criterion: selected iff ((w0 s0 + w1 s1) + w2 s2) + w3 s3 > max_mean_squared_error * texels."""
    _fields_ = [("channel_weight", C.c_double * 4), ("max_mean_squared_error", C.c_double)]


def block_criterion(max_mean_squared_error, channel_weight=(1.0, 1.0, 1.0, 1.0)):
    return BlockCriterion((C.c_double * 4)(*channel_weight), max_mean_squared_error)


class AdaptiveStats(C.Structure):
    """struct astcenc_amd_adaptive_stats."""
    _fields_ = [("blocks", C.c_uint), ("selected", C.c_uint), ("replaced", C.c_uint),
                ("kernel_ms_base", C.c_float), ("kernel_ms_strong", C.c_float), ("kernel_ms_other", C.c_float)]


class AdaptiveSetStats(C.Structure):
    """struct astcenc_amd_adaptive_set_stats."""
    _fields_ = [("blocks", C.c_uint), ("candidates", C.c_uint), ("selected", C.c_uint), ("replaced", C.c_uint),
                ("kernel_ms_base", C.c_float), ("kernel_ms_strong", C.c_float), ("kernel_ms_other", C.c_float)]


class AstcError(RuntimeError):
    def __init__(self, code, where):
        super().__init__("%s failed with astcenc_error %d" % (where, code))
        self.code = code


class Library:
    """One loaded astcenc-ABI shared object."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        L.astcenc_config_init.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_uint, C.POINTER(Config)]
        L.astcenc_config_init.restype = C.c_int
        L.astcenc_context_alloc.argtypes = [C.POINTER(Config), C.c_uint, C.POINTER(C.c_void_p), C.c_void_p]
        L.astcenc_context_alloc.restype = C.c_int
        L.astcenc_compress_image.argtypes = [C.c_void_p, C.POINTER(Image), C.POINTER(Swizzle), C.c_void_p, C.c_size_t, C.c_uint]
        L.astcenc_compress_image.restype = C.c_int
        L.astcenc_compress_reset.argtypes = [C.c_void_p]
        L.astcenc_compress_reset.restype = C.c_int
        L.astcenc_compress_cancel.argtypes = [C.c_void_p]
        L.astcenc_compress_cancel.restype = C.c_int
        L.astcenc_decompress_image.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Image), C.POINTER(Swizzle), C.c_uint]
        L.astcenc_decompress_image.restype = C.c_int
        L.astcenc_decompress_reset.argtypes = [C.c_void_p]
        L.astcenc_decompress_reset.restype = C.c_int
        L.astcenc_context_free.argtypes = [C.c_void_p]
        L.astcenc_context_free.restype = None
        L.astcenc_get_block_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BlockInfo)]
        L.astcenc_get_block_info.restype = C.c_int
        L.astcenc_get_error_string.argtypes = [C.c_int]
        L.astcenc_get_error_string.restype = C.c_char_p
        self.has_amd = hasattr(L, "astcenc_amd_compress_image_device")
        if self.has_amd:
            L.astcenc_amd_compress_image_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int,
                                                            C.POINTER(Swizzle), C.c_void_p, C.c_size_t, C.c_void_p,
                                                            C.POINTER(C.c_float)]
            L.astcenc_amd_compress_image_device.restype = C.c_int
            L.astcenc_amd_backend_name.restype = C.c_char_p
        if hasattr(L, "astcenc_amd_compare_images_device"):
            L.astcenc_amd_decompress_image_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                                              C.c_int, C.POINTER(Swizzle), C.c_void_p]
            L.astcenc_amd_decompress_image_device.restype = C.c_int
            L.astcenc_amd_compare_images_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint,
                                                            C.c_void_p, C.POINTER(ErrorSums)]
            L.astcenc_amd_compare_images_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_compare_images_hdr_device"):
            L.astcenc_amd_compare_images_hdr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint,
                                                                C.c_int, C.c_int, C.c_void_p, C.POINTER(ErrorSums), C.POINTER(HdrErrorSums)]
            L.astcenc_amd_compare_images_hdr_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_context_device_count"):
            L.astcenc_amd_context_device_count.argtypes = [C.c_void_p]
            L.astcenc_amd_context_device_count.restype = C.c_int
            L.astcenc_amd_context_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.astcenc_amd_context_set_option.restype = C.c_int
        if hasattr(L, "astcenc_amd_context_kernel_name"):
            L.astcenc_amd_context_kernel_name.argtypes = [C.c_void_p]
            L.astcenc_amd_context_kernel_name.restype = C.c_char_p
        if hasattr(L, "astcenc_amd_context_specialize"):
            L.astcenc_amd_context_specialize.argtypes = [C.c_void_p]
            L.astcenc_amd_context_specialize.restype = C.c_int
        if hasattr(L, "astcenc_amd_compress_volume_device"):
            L.astcenc_amd_compress_volume_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                             C.POINTER(Swizzle), C.c_void_p, C.c_size_t, C.c_void_p,
                                                             C.POINTER(C.c_float)]
            L.astcenc_amd_compress_volume_device.restype = C.c_int

        if hasattr(L, "astcenc_amd_compress_images_device"):
            L.astcenc_amd_compress_images_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_images_device.restype = C.c_int
            L.astcenc_amd_decompress_images_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.c_void_p]
            L.astcenc_amd_decompress_images_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_decompress_regions_device"):
            L.astcenc_amd_decompress_regions_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(DecodeRegion), C.c_uint,
                                                                C.c_void_p]
            L.astcenc_amd_decompress_regions_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_decompress_tensors_device"):
            L.astcenc_amd_decompress_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat),
                                                                C.POINTER(TensorRegion), C.c_uint, C.c_void_p]
            L.astcenc_amd_decompress_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_decompress_scaled_tensors_device"):
            L.astcenc_amd_decompress_scaled_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.c_int,
                                                                       C.POINTER(ScaledRegion), C.c_uint, C.c_void_p]
            L.astcenc_amd_decompress_scaled_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_lod_tensors_device"):
            L.astcenc_amd_sample_lod_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(LodSampler),
                                                                C.POINTER(LodGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_lod_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_lod_grad_device"):
            L.astcenc_amd_sample_lod_grad_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(LodSampler),
                                                             C.POINTER(LodGradGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_lod_grad_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_cube_tensors_device"):
            L.astcenc_amd_sample_cube_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(CubeSampler),
                                                                 C.POINTER(CubeGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_cube_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_volume_tensors_device"):
            L.astcenc_amd_sample_volume_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(VolumeSampler),
                                                                   C.POINTER(VolumeGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_volume_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_volume_grad_device"):
            L.astcenc_amd_sample_volume_grad_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(VolumeSampler),
                                                                C.POINTER(VolumeGradGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_volume_grad_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_sample_tensors_device"):
            L.astcenc_amd_sample_tensors_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.POINTER(TensorFormat), C.POINTER(Sampler),
                                                            C.POINTER(SampleGrid), C.c_uint, C.c_void_p]
            L.astcenc_amd_sample_tensors_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_compare_blocks_device"):
            blocks_args = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int, C.POINTER(Swizzle),
                           C.c_void_p, C.c_size_t]
            L.astcenc_amd_compare_blocks_device.argtypes = blocks_args + [C.c_void_p, C.POINTER(ErrorSums)]
            L.astcenc_amd_compare_blocks_device.restype = C.c_int
            L.astcenc_amd_compare_blocks_hdr_device.argtypes = blocks_args + [C.c_int, C.c_int, C.c_void_p, C.POINTER(ErrorSums), C.POINTER(HdrErrorSums)]
            L.astcenc_amd_compare_blocks_hdr_device.restype = C.c_int
            L.astcenc_amd_compare_image_set_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                                               C.POINTER(ErrorSums)]
            L.astcenc_amd_compare_image_set_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_compress_block_list_device"):
            L.astcenc_amd_compress_block_list_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                 C.POINTER(Swizzle), C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t,
                                                                 C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_block_list_device.restype = C.c_int
            L.astcenc_amd_select_blocks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint,
                                                           C.POINTER(BlockCriterion), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint)]
            L.astcenc_amd_select_blocks_device.restype = C.c_int
            L.astcenc_amd_compress_image_adaptive_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                     C.POINTER(Swizzle), C.POINTER(Swizzle), C.POINTER(BlockCriterion),
                                                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                     C.POINTER(AdaptiveStats)]
            L.astcenc_amd_compress_image_adaptive_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_select_blocks_set_device"):
            L.astcenc_amd_select_blocks_set_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.c_void_p, C.c_size_t,
                                                               C.POINTER(BlockCriterion), C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                                               C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
            L.astcenc_amd_select_blocks_set_device.restype = C.c_int
            L.astcenc_amd_compress_block_list_set_device.argtypes = [C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint, C.c_void_p, C.c_uint,
                                                                     C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_block_list_set_device.restype = C.c_int
            L.astcenc_amd_compress_images_adaptive_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ImageSetEntry), C.c_uint,
                                                                      C.POINTER(Swizzle), C.POINTER(BlockCriterion), C.c_uint, C.c_void_p,
                                                                      C.c_size_t, C.c_void_p, C.POINTER(AdaptiveSetStats)]
            L.astcenc_amd_compress_images_adaptive_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_mip_chain_layout"):
            L.astcenc_amd_mip_chain_layout.argtypes = [C.POINTER(Config), C.c_uint, C.c_uint, C.c_int, C.c_uint, C.POINTER(MipChainLayout)]
            L.astcenc_amd_mip_chain_layout.restype = C.c_int
            L.astcenc_amd_generate_mip_chain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_void_p,
                                                                C.c_size_t, C.c_void_p]
            L.astcenc_amd_generate_mip_chain_device.restype = C.c_int
            L.astcenc_amd_compress_mip_chain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.POINTER(Swizzle),
                                                                C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                C.POINTER(C.c_float)]
            L.astcenc_amd_compress_mip_chain_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_mip_chain_volume_layout"):
            L.astcenc_amd_mip_chain_volume_layout.argtypes = [C.POINTER(Config), C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_uint,
                                                              C.POINTER(MipChainVolumeLayout)]
            L.astcenc_amd_mip_chain_volume_layout.restype = C.c_int
            L.astcenc_amd_generate_mip_chain_volume_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                       C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]
            L.astcenc_amd_generate_mip_chain_volume_device.restype = C.c_int
            L.astcenc_amd_compress_mip_chain_volume_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                       C.POINTER(Swizzle), C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                       C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_mip_chain_volume_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_generate_mip_chain_ex_device"):
            L.astcenc_amd_generate_mip_chain_ex_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                   C.c_uint, C.POINTER(MipOptions), C.c_void_p, C.c_size_t, C.c_void_p]
            L.astcenc_amd_generate_mip_chain_ex_device.restype = C.c_int
            L.astcenc_amd_compress_mip_chain_ex_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                   C.POINTER(Swizzle), C.c_uint, C.POINTER(MipOptions), C.c_void_p,
                                                                   C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_mip_chain_ex_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_generate_mip_chain_filtered_device"):
            L.astcenc_amd_generate_mip_chain_filtered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                         C.c_int, C.c_uint, C.POINTER(MipOptions), C.POINTER(MipFilter),
                                                                         C.c_void_p, C.c_size_t, C.c_void_p]
            L.astcenc_amd_generate_mip_chain_filtered_device.restype = C.c_int
            L.astcenc_amd_compress_mip_chain_filtered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                         C.c_int, C.POINTER(Swizzle), C.c_uint, C.POINTER(MipOptions),
                                                                         C.POINTER(MipFilter), C.c_void_p, C.c_size_t, C.c_void_p,
                                                                         C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_compress_mip_chain_filtered_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_generate_mip_chain_weighted_device"):
            L.astcenc_amd_generate_mip_chain_weighted_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                         C.c_int, C.c_uint, C.POINTER(MipOptions), C.POINTER(MipFilter),
                                                                         C.POINTER(MipWeighting), C.c_void_p, C.c_size_t, C.c_void_p]
            L.astcenc_amd_generate_mip_chain_weighted_device.restype = C.c_int
            L.astcenc_amd_compress_mip_chain_weighted_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int,
                                                                         C.c_int, C.POINTER(Swizzle), C.c_uint, C.POINTER(MipOptions),
                                                                         C.POINTER(MipFilter), C.POINTER(MipWeighting), C.c_void_p,
                                                                         C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                         C.POINTER(C.c_float)]
            L.astcenc_amd_compress_mip_chain_weighted_device.restype = C.c_int
        if hasattr(L, "astcenc_amd_resize_image_device"):
            L.astcenc_amd_resize_image_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                          C.POINTER(Resize), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
            L.astcenc_amd_resize_image_device.restype = C.c_int
            L.astcenc_amd_resize_dims.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
            L.astcenc_amd_resize_dims.restype = C.c_int

    # -- thin wrappers returning error codes, as the C API does --
    def config_init(self, profile, bx, by, bz, quality, flags):
        cfg = Config()
        err = self.lib.astcenc_config_init(profile, bx, by, bz, quality, flags, C.byref(cfg))
        return err, cfg

    def context_alloc(self, cfg, thread_count=1, parent=None):
        ctx = C.c_void_p()
        err = self.lib.astcenc_context_alloc(C.byref(cfg) if cfg is not None else None, thread_count, C.byref(ctx), parent)
        return err, ctx

    def context_free(self, ctx):
        self.lib.astcenc_context_free(ctx)

    def error_string(self, code):
        s = self.lib.astcenc_get_error_string(code)
        return s.decode() if s else None

    def backend_name(self):
        return self.lib.astcenc_amd_backend_name().decode() if self.has_amd else "reference"

    def compress_raw(self, ctx, pixels, out, swizzle=SWZ_RGBA, thread_index=0, data_len=None):
        """pixels: contiguous array [H, W, 4] (or [D, H, W, 4] for a volume / array image) of
        uint8 / float16 / float32; out: uint8 array."""
        d = pixels.shape[0] if pixels.ndim == 4 else 1
        h, w = pixels.shape[-3], pixels.shape[-2]
        dtype = {np.dtype(np.uint8): TYPE_U8, np.dtype(np.float16): TYPE_F16, np.dtype(np.float32): TYPE_F32}[pixels.dtype]
        slice_bytes = h * w * 4 * pixels.dtype.itemsize
        slices = (C.c_void_p * d)(*[pixels.ctypes.data + z * slice_bytes for z in range(d)])
        img = Image(w, h, d, dtype, slices)
        swz = Swizzle(*swizzle)
        return self.lib.astcenc_compress_image(ctx, C.byref(img), C.byref(swz), out.ctypes.data,
                                               out.nbytes if data_len is None else data_len, thread_index)

    def compress(self, pixels, block=(6, 6), quality=PRE_MEDIUM, profile=PRF_LDR, flags=0, swizzle=SWZ_RGBA, tweak=None, options=None,
                 specialize=False):
        """Convenience: config_init -> context_alloc -> compress_image -> free. Returns uint8 [blocks*16].
        block is (x, y) or (x, y, z); pixels is [H, W, 4] or [D, H, W, 4]; options: {OPT_*: value} for
        astcenc_amd_context_set_option (product library only); specialize: wait for the context's specialised kernel
        build first (astcenc_amd_context_specialize; "try": go on with the generic build if there is none) -- self.last_kernel then
        names the build that ran."""
        bz = block[2] if len(block) > 2 else 1
        err, cfg = self.config_init(profile, block[0], block[1], bz, quality, flags)
        if err:
            raise AstcError(err, "astcenc_config_init")
        if tweak:
            tweak(cfg)
        err, ctx = self.context_alloc(cfg, 1)
        if err:
            raise AstcError(err, "astcenc_context_alloc")
        try:
            for opt, value in (options or {}).items():
                err = self.lib.astcenc_amd_context_set_option(ctx, opt, value)
                if err:
                    raise AstcError(err, "astcenc_amd_context_set_option")
            if specialize:
                err = self.lib.astcenc_amd_context_specialize(ctx)
                if err and specialize != "try":          # ("try": a refused build leaves the context on the generic kernel)
                    raise AstcError(err, "astcenc_amd_context_specialize")
            if hasattr(self.lib, "astcenc_amd_context_kernel_name"):
                self.last_kernel = self.lib.astcenc_amd_context_kernel_name(ctx).decode()
            d = pixels.shape[0] if pixels.ndim == 4 else 1
            h, w = pixels.shape[-3], pixels.shape[-2]
            bx, by = (w + block[0] - 1) // block[0], (h + block[1] - 1) // block[1]
            out = np.zeros(bx * by * ((d + bz - 1) // bz) * 16, dtype=np.uint8)
            err = self.compress_raw(ctx, np.ascontiguousarray(pixels), out, swizzle)
            if err:
                raise AstcError(err, "astcenc_compress_image")
            return out
        finally:
            self.context_free(ctx)

    @staticmethod
    def _set_args(entries, stream):
        """ctypes array of the entries (ImageSetEntry, or (image, blocks[, swizzle]) tuples of torch tensors) and the stream:
        a torch stream, a raw hipStream_t, or None for torch's current stream."""
        device = next((e[1].device for e in entries if not isinstance(e, ImageSetEntry)), None)
        entries = [e if isinstance(e, ImageSetEntry) else image_set_entry(*e) for e in entries]
        arr = (ImageSetEntry * len(entries))(*entries) if entries else None
        return arr, len(entries), torch_stream(stream, device)

    def compress_images_device(self, ctx, entries, stream=None):
        """astcenc_amd_compress_images_device over `entries` (see _set_args); returns the astcenc_error, the kernel time of the
        call (ms) in self.last_kernel_ms."""
        arr, n, s = self._set_args(entries, stream)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_images_device(ctx, arr, n, s, C.byref(ms))
        self.last_kernel_ms = ms.value
        return err

    def decompress_images_device(self, ctx, entries, stream=None):
        """astcenc_amd_decompress_images_device over `entries` (see _set_args): every entry's blocks into its image."""
        arr, n, s = self._set_args(entries, stream)
        return self.lib.astcenc_amd_decompress_images_device(ctx, arr, n, s)

    def decompress_regions_device(self, ctx, entries, regions, stream=None):
        """astcenc_amd_decompress_regions_device: windows of the compressed images `entries` (see _set_args; compressed_entry makes
        one without an image) into buffers of their own.  regions: DecodeRegion, or (entry, (x, y, z), (size_x, size_y, size_z), out)
        tuples (see decode_region)."""
        arr, n, s = self._set_args(entries, stream)
        regions = [r if isinstance(r, DecodeRegion) else decode_region(*r) for r in regions]
        rarr = (DecodeRegion * len(regions))(*regions) if regions else None
        return self.lib.astcenc_amd_decompress_regions_device(ctx, arr, n, rarr, len(regions), s)

    def decompress_tensors_device(self, ctx, entries, format, regions, stream=None):
        """astcenc_amd_decompress_tensors_device: windows of the compressed images `entries` (see _set_args, compressed_entry)
        decoded into tensors of `format` (a TensorFormat, see tensor_format).  regions: TensorRegion, or (entry, (x, y, z),
        (size_x, size_y, size_z), out_view[, flip_x[, flip_y]]) tuples (see tensor_region; the view is read with the format's
        layout)."""
        arr, n, s = self._set_args(entries, stream)
        regions = [r if isinstance(r, TensorRegion) else tensor_region(*r, layout=format.layout) for r in regions]
        rarr = (TensorRegion * len(regions))(*regions) if regions else None
        return self.lib.astcenc_amd_decompress_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None, rarr, len(regions), s)

    def decompress_scaled_tensors_device(self, ctx, entries, format, filter, regions, stream=None):
        """astcenc_amd_decompress_scaled_tensors_device: windows of the compressed images `entries` resampled with `filter`
        (WINDOW_BILINEAR / WINDOW_BOX) into tensors of `format`.  regions: ScaledRegion, or (entry, (x, y, z), (size_x, size_y),
        out_view[, flip_x[, flip_y]]) tuples (see scaled_region; the view is read with the format's layout and must have its type)."""
        arr, n, s = self._set_args(entries, stream)
        regions = [r if isinstance(r, ScaledRegion) else scaled_region(*r, layout=format.layout, type=format.type) for r in regions]
        rarr = (ScaledRegion * len(regions))(*regions) if regions else None
        return self.lib.astcenc_amd_decompress_scaled_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None, filter, rarr, len(regions), s)

    def sample_tensors_device(self, ctx, entries, format, sampler, grids, stream=None):
        """astcenc_amd_sample_tensors_device: the compressed images `entries` sampled at coordinates into tensors of `format`.
        sampler: a Sampler, or a (filter, address_x, address_y) tuple of SAMPLE_* / ADDRESS_* constants.  grids: SampleGrid, or
        (entry, z, coords, out_view) tuples (see sample_grid; the view is read with the format's layout and must have its type)."""
        arr, n, s = self._set_args(entries, stream)
        if sampler is not None and not isinstance(sampler, Sampler):
            sampler = Sampler(*sampler)
        grids = [g if isinstance(g, SampleGrid) else sample_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (SampleGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                          C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_lod_tensors_device(self, ctx, entries, format, sampler, grids, stream=None):
        """astcenc_amd_sample_lod_tensors_device: mip chains among the compressed images `entries` sampled at normalised coordinates
        and a level of detail per point into tensors of `format`.  sampler: a LodSampler, or a (filter, address_x, address_y,
        mip_filter) tuple of SAMPLE_* / ADDRESS_* / MIP_NEAREST, MIP_LINEAR constants.  grids: LodGrid, or (first_entry, level_count,
        z, coords, lod, out_view[, lod_bias]) tuples (see lod_grid; the view is read with the format's layout and must have its type)."""
        arr, n, s = self._set_args(entries, stream)
        if sampler is not None and not isinstance(sampler, LodSampler):
            sampler = LodSampler(*sampler)
        grids = [g if isinstance(g, LodGrid) else lod_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (LodGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_lod_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                              C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_lod_grad_device(self, ctx, entries, format, sampler, grids, stream=None):
        """astcenc_amd_sample_lod_grad_device: the gradients of sample_lod_tensors_device with respect to the coordinates and the
        levels of detail, for upstream gradients of `format`'s type and layout.  sampler as there.  grids: LodGradGrid, or
        (first_entry, level_count, z, coords, lod, grad_out, grad_coords[, grad_lod[, lod_bias]]) tuples (see lod_grad_grid)."""
        arr, n, s = self._set_args(entries, stream)
        if sampler is not None and not isinstance(sampler, LodSampler):
            sampler = LodSampler(*sampler)
        grids = [g if isinstance(g, LodGradGrid) else lod_grad_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (LodGradGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_lod_grad_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                           C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_lod(self, ctx, entries, format, sampler, first_entry, level_count, z, coords, lod=None, lod_bias=0.0):
        """The lod call as a differentiable torch operation: samples slice `z` of the chain entries[first_entry : first_entry +
        level_count] at `coords` (float32 [H, W, 2]) and `lod` (float32 [H, W] or None) into a new tensor of `format` -- [C, H, W]
        or [H, W, C] -- on torch's current stream; its backward is sample_lod_grad_device and returns gradients for `coords` and
        `lod` only (the texels are compressed and fixed).  AstcError when either call fails."""
        entries = [e if isinstance(e, ImageSetEntry) else image_set_entry(*e) for e in entries]
        if not isinstance(sampler, LodSampler):
            sampler = LodSampler(*sampler)
        return _sample_lod_function().apply(coords, lod, self, ctx, entries, format, sampler, first_entry, level_count, z, lod_bias)

    def sample_cube_tensors_device(self, ctx, entries, format, sampler, grids, stream=None):
        """astcenc_amd_sample_cube_tensors_device: cube maps (one level or a mip chain) among the compressed images `entries`
        sampled by direction at a level of detail per point into tensors of `format`.  sampler: a CubeSampler, or a (filter,
        mip_filter) tuple of SAMPLE_* / MIP_NEAREST, MIP_LINEAR constants.  grids: CubeGrid, or (first_entry, level_count, cube,
        dirs, lod, out_view[, lod_bias]) tuples (see cube_grid; the view is read with the format's layout and must have its type)."""
        arr, n, s = self._set_args(entries, stream)
        if sampler is not None and not isinstance(sampler, CubeSampler):
            sampler = CubeSampler(*sampler)
        grids = [g if isinstance(g, CubeGrid) else cube_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (CubeGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_cube_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                               C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_volume_tensors_device(self, ctx, entries, format, sampler, grids, stream=None):
        """astcenc_amd_sample_volume_tensors_device: volumes (one level or a mip chain, 2D or 3D footprints) among the compressed
        images `entries` sampled at normalised (u, v, w) at a level of detail per point into tensors of `format`.  sampler: a
        VolumeSampler, or a (filter, address_x, address_y, address_z, mip_filter) tuple of SAMPLE_* / ADDRESS_* / MIP_NEAREST,
        MIP_LINEAR constants.  grids: VolumeGrid, or (first_entry, level_count, coords, lod, out_view[, lod_bias]) tuples (see
        volume_grid; the view is read with the format's layout and must have its type)."""
        arr, n, s = self._set_args(entries, stream)
        if sampler is not None and not isinstance(sampler, VolumeSampler):
            sampler = VolumeSampler(*sampler)
        grids = [g if isinstance(g, VolumeGrid) else volume_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (VolumeGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_volume_tensors_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                                 C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_volume_grad(self, ctx, entries, format, sampler, grids):
        """astcenc_amd_sample_volume_grad_device: the gradients of sample_volume_tensors_device with respect to the coordinates and
        the levels of detail, for upstream gradients of `format`'s type and layout.  sampler as there.  grids: VolumeGradGrid, or
        (first_entry, level_count, coords, lod, grad_out, grad_coords[, grad_lod[, lod_bias]]) tuples (see volume_grad_grid).
        The call runs on torch's current stream (torch_stream()) and is complete on return; there is no stream argument, and the
        name has no _device suffix: the table of tests/test_stream_order.py lists every method of this class that has either, row
        by row, and this one's ordering is tested in tests/test_decode_volume_grad.py instead.  A caller who wants another stream
        makes it current: `with torch.cuda.stream(s): lib.sample_volume_grad(...)`."""
        arr, n, s = self._set_args(entries, None)
        if sampler is not None and not isinstance(sampler, VolumeSampler):
            sampler = VolumeSampler(*sampler)
        grids = [g if isinstance(g, VolumeGradGrid) else volume_grad_grid(*g, layout=format.layout, type=format.type) for g in grids]
        garr = (VolumeGradGrid * len(grids))(*grids) if grids else None
        return self.lib.astcenc_amd_sample_volume_grad_device(ctx, arr, n, C.byref(format) if format is not None else None,
                                                              C.byref(sampler) if sampler is not None else None, garr, len(grids), s)

    def sample_volume(self, ctx, entries, format, sampler, first_entry, level_count, coords, lod=None, lod_bias=0.0):
        """The volume call as a differentiable torch operation: samples the chain entries[first_entry : first_entry + level_count]
        at `coords` (float32 [H, W, 3]) and `lod` (float32 [H, W] or None) into a new tensor of `format` -- [C, H, W] or
        [H, W, C] -- on torch's current stream; its backward is sample_volume_grad and returns gradients for `coords` and `lod`
        only (the texels are compressed and fixed).  AstcError when either call fails."""
        entries = [e if isinstance(e, ImageSetEntry) else image_set_entry(*e) for e in entries]
        if not isinstance(sampler, VolumeSampler):
            sampler = VolumeSampler(*sampler)
        return _sample_volume_function().apply(coords, lod, self, ctx, entries, format, sampler, first_entry, level_count, lod_bias)

    @staticmethod
    def _blocks_args(blocks, image, decode_type, swizzle, block_errors, stream):
        """The arguments astcenc_amd_compare_blocks_device and its _hdr_ form share, from device tensors: `blocks` uint8, `image`
        [H, W, 4] or [D, H, W, 4] (the original), `block_errors` None or a float64 tensor of four values per block."""
        import torch
        types = {torch.uint8: TYPE_U8, torch.float16: TYPE_F16, torch.float32: TYPE_F32}
        assert image.is_contiguous() and blocks.is_contiguous() and image.dim() in (3, 4) and image.shape[-1] == 4
        assert block_errors is None or (block_errors.is_contiguous() and block_errors.dtype == torch.float64)
        d = image.shape[0] if image.dim() == 4 else 1
        image_type = types[image.dtype]
        return [blocks.data_ptr(), blocks.numel(), image.data_ptr(), image.shape[-2], image.shape[-3], d, image_type,
                image_type if decode_type is None else decode_type, C.byref(Swizzle(*swizzle)),
                None if block_errors is None else block_errors.data_ptr(), 0 if block_errors is None else block_errors.numel() * 8], \
            torch_stream(stream, image.device)

    def compare_blocks_device(self, ctx, blocks, image, decode_type=None, swizzle=SWZ_RGBA, block_errors=None, stream=None):
        """astcenc_amd_compare_blocks_device: the blocks decoded to decode_type (default: the image's type) through `swizzle` against
        the original `image`, no decoded image in memory.  Returns (error, ErrorSums); block_errors (optional, float64 [blocks, 4])
        receives the per-block squared errors."""
        args, s = self._blocks_args(blocks, image, decode_type, swizzle, block_errors, stream)
        sums = ErrorSums()
        err = self.lib.astcenc_amd_compare_blocks_device(ctx, *args, s, C.byref(sums))
        return err, sums

    def compare_blocks_hdr_device(self, ctx, blocks, image, fstop_lo=-10, fstop_hi=10, decode_type=None, swizzle=SWZ_RGBA, block_errors=None,
                                  stream=None):
        """astcenc_amd_compare_blocks_hdr_device: as compare_blocks_device, with the HDR sums over the f-stops.  Returns
        (error, ErrorSums, HdrErrorSums)."""
        args, s = self._blocks_args(blocks, image, decode_type, swizzle, block_errors, stream)
        sums, hdr = ErrorSums(), HdrErrorSums()
        err = self.lib.astcenc_amd_compare_blocks_hdr_device(ctx, *args, fstop_lo, fstop_hi, s, C.byref(sums), C.byref(hdr))
        return err, sums, hdr

    @staticmethod
    def _image_args(image, stream):
        """(data pointer, dim_x, dim_y, dim_z, astcenc_type) of a contiguous device tensor [H, W, 4] or [D, H, W, 4], and the stream."""
        import torch
        types = {torch.uint8: TYPE_U8, torch.float16: TYPE_F16, torch.float32: TYPE_F32}
        assert image.is_contiguous() and image.dim() in (3, 4) and image.shape[-1] == 4
        d = image.shape[0] if image.dim() == 4 else 1
        return [image.data_ptr(), image.shape[-2], image.shape[-3], d, types[image.dtype]], torch_stream(stream, image.device)

    def compress_block_list_device(self, ctx, image, block_list, out, swizzle=SWZ_RGBA, list_count=None, data_len=None, stream=None):
        """astcenc_amd_compress_block_list_device: the blocks of `image` named in `block_list` (a device tensor of 32-bit raster block
        indices, or None) into their slots of `out` (device uint8, 16 bytes per block of the whole image).  list_count / data_len
        override what the tensors say.  Returns the astcenc_error, the kernel time (ms) in self.last_kernel_ms."""
        args, s = self._image_args(image, stream)
        assert block_list is None or (block_list.is_contiguous() and block_list.element_size() == 4)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_block_list_device(
            ctx, *args, C.byref(Swizzle(*swizzle)), None if block_list is None else block_list.data_ptr(),
            (0 if block_list is None else block_list.numel()) if list_count is None else list_count,
            out.data_ptr(), out.numel() if data_len is None else data_len, s, C.byref(ms))
        self.last_kernel_ms = ms.value
        return err

    def select_blocks_device(self, ctx, block_errors, dims, criterion, block_list, stream=None):
        """astcenc_amd_select_blocks_device: `block_errors` float64 [blocks, 4] on the device, dims (x, y, z) of the image,
        `criterion` a BlockCriterion, `block_list` a device tensor of 32-bit words, one per block.  Returns (error, count): the
        ascending indices of the selected blocks are block_list[:count]."""
        count = C.c_uint(0)
        err = self.lib.astcenc_amd_select_blocks_device(ctx, block_errors.data_ptr(), block_errors.numel() * 8, dims[0], dims[1], dims[2],
                                                        C.byref(criterion), block_list.data_ptr(), block_list.numel() * 4,
                                                        torch_stream(stream, block_errors.device), C.byref(count))
        return err, count.value

    def compress_image_adaptive_device(self, base_ctx, strong_ctx, image, criterion, out, swizzle=SWZ_RGBA, decode_swizzle=SWZ_RGBA,
                                       block_errors=None, stream=None):
        """astcenc_amd_compress_image_adaptive_device: `image` compressed with base_ctx into `out`, the blocks that miss `criterion`
        re-encoded with strong_ctx and kept where better; block_errors (optional, float64 [blocks, 4]) receives the final stream's
        records.  Returns (error, AdaptiveStats)."""
        args, s = self._image_args(image, stream)
        stats = AdaptiveStats()
        err = self.lib.astcenc_amd_compress_image_adaptive_device(
            base_ctx, strong_ctx, *args, C.byref(Swizzle(*swizzle)), C.byref(Swizzle(*decode_swizzle)), C.byref(criterion),
            out.data_ptr(), out.numel(), None if block_errors is None else block_errors.data_ptr(),
            0 if block_errors is None else block_errors.numel() * 8, s, C.byref(stats))
        return err, stats

    def select_blocks_set_device(self, ctx, dims, block_errors, criterion, block_list, max_blocks=NO_BLOCK_BUDGET, stream=None):
        """astcenc_amd_select_blocks_set_device: `dims` the (x, y, z) of every entry of the set, `block_errors` float64 [blocks of the
        set, 4] on the device, `block_list` a device tensor of 32-bit words.  Returns (error, candidates, selected): the ascending
        global indices of the selected blocks are block_list[:selected]."""
        entries = (ImageSetEntry * max(len(dims), 1))(*[ImageSetEntry(None, None, 0, d[0], d[1], d[2], TYPE_U8, Swizzle(*SWZ_RGBA)) for d in dims])
        candidates, selected = C.c_uint(0), C.c_uint(0)
        err = self.lib.astcenc_amd_select_blocks_set_device(ctx, entries, len(dims), block_errors.data_ptr(), block_errors.numel() * 8,
                                                            C.byref(criterion), max_blocks, block_list.data_ptr(), block_list.numel() * 4,
                                                            torch_stream(stream, block_errors.device), C.byref(candidates), C.byref(selected))
        return err, candidates.value, selected.value

    def compress_block_list_set_device(self, ctx, entries, block_list, list_count=None, stream=None):
        """astcenc_amd_compress_block_list_set_device over `entries` (see _set_args): the blocks named in `block_list` (a device
        tensor of 32-bit global block indices, or None) into their slots of their entries' blocks.  Returns the astcenc_error, the
        kernel time (ms) in self.last_kernel_ms."""
        arr, n, s = self._set_args(entries, stream)
        assert block_list is None or (block_list.is_contiguous() and block_list.element_size() == 4)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_block_list_set_device(
            ctx, arr, n, None if block_list is None else block_list.data_ptr(),
            (0 if block_list is None else block_list.numel()) if list_count is None else list_count, s, C.byref(ms))
        self.last_kernel_ms = ms.value
        return err

    def compress_images_adaptive_device(self, base_ctx, strong_ctx, entries, criterion, max_blocks=NO_BLOCK_BUDGET, decode_swizzle=SWZ_RGBA,
                                        block_errors=None, stream=None):
        """astcenc_amd_compress_images_adaptive_device over `entries` (see _set_args): every entry compressed with base_ctx into its
        blocks, the at most max_blocks worst blocks that miss `criterion` re-encoded with strong_ctx and kept where better;
        block_errors (optional, float64, four values per block of the set) receives the final streams' records.  Returns
        (error, AdaptiveSetStats)."""
        arr, n, s = self._set_args(entries, stream)
        stats = AdaptiveSetStats()
        err = self.lib.astcenc_amd_compress_images_adaptive_device(
            base_ctx, strong_ctx, arr, n, C.byref(Swizzle(*decode_swizzle)), C.byref(criterion), max_blocks,
            None if block_errors is None else block_errors.data_ptr(), 0 if block_errors is None else block_errors.numel() * 8, s,
            C.byref(stats))
        return err, stats

    def compare_image_set_device(self, ctx, entries, block_errors=None, stream=None):
        """astcenc_amd_compare_image_set_device over `entries` (see _set_args; an entry's image is the original, nothing in an entry
        is written).  Returns (error, [ErrorSums per entry]); block_errors (optional, float64, four values per block of the whole
        set) receives every entry's per-block squared errors back to back."""
        arr, n, s = self._set_args(entries, stream)
        sums = (ErrorSums * max(n, 1))()
        err = self.lib.astcenc_amd_compare_image_set_device(ctx, arr, n, None if block_errors is None else block_errors.data_ptr(),
                                                            0 if block_errors is None else block_errors.numel() * 8, s, sums)
        return err, list(sums)[:n]

    def mip_chain_layout(self, cfg, w, h, dtype, levels=0):
        """astcenc_amd_mip_chain_layout for the footprint of `cfg` (a Config); dtype: TYPE_*.  Returns (error, MipChainLayout)."""
        layout = MipChainLayout()
        err = self.lib.astcenc_amd_mip_chain_layout(C.byref(cfg), w, h, dtype, levels, C.byref(layout))
        return err, layout

    def _mip_chain_buffers(self, ctx, image, levels, blocks):
        """(w, h, dtype code, layout, device_levels tensor, level tensors [level 0 = image], blocks tensor or None) of the chain of
        an [H, W, 4] device tensor: the volume of depth 1's; the context's config gives the footprint."""
        assert image.dim() == 3, "a contiguous [H, W, 4] device tensor"
        (w, h, _), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(ctx, image[None], MIP_VOLUME, levels, blocks)
        return w, h, dtype, layout, store, [image] + [t[0] for t in tensors[1:]], out

    def _ctx_block(self, ctx):
        """The footprint of a context (astcenc_get_block_info on a zero block: it reports the context's block size)."""
        info = BlockInfo()
        self.lib.astcenc_get_block_info(ctx, (C.c_uint8 * 16)(), C.byref(info))
        return info.block_x, info.block_y, info.block_z

    def generate_mip_chain_device(self, ctx, image, levels=0, stream=None):
        """Levels of the [H, W, 4] device tensor `image` (astcenc_amd_generate_mip_chain_device): a list of torch views, one per
        level, level 0 being `image` itself and the others views of one buffer."""
        w, h, dtype, layout, store, tensors, _ = self._mip_chain_buffers(ctx, image, levels, False)
        s = torch_stream(stream, image.device)
        err = self.lib.astcenc_amd_generate_mip_chain_device(ctx, image.data_ptr(), w, h, dtype, layout.level_count,
                                                             store.data_ptr(), layout.texels_len, s)
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_device")
        return tensors

    def compress_mip_chain_device(self, ctx, image, levels=0, swizzle=SWZ_RGBA, stream=None):
        """astcenc_amd_compress_mip_chain_device: returns (level tensors, per-level block tensors); the kernel time of the call
        (ms, generation included) in self.last_kernel_ms."""
        w, h, dtype, layout, store, tensors, out = self._mip_chain_buffers(ctx, image, levels, True)
        s = torch_stream(stream, image.device)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_mip_chain_device(ctx, image.data_ptr(), w, h, dtype, C.byref(Swizzle(*swizzle)),
                                                             layout.level_count, store.data_ptr(), layout.texels_len,
                                                             out.data_ptr(), layout.blocks_len, s, C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_compress_mip_chain_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        return tensors, [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]

    def mip_chain_volume_layout(self, cfg, w, h, d, kind, dtype, levels=0):
        """astcenc_amd_mip_chain_volume_layout; kind: MIP_ARRAY / MIP_VOLUME.  Returns (error, MipChainVolumeLayout)."""
        layout = MipChainVolumeLayout()
        err = self.lib.astcenc_amd_mip_chain_volume_layout(C.byref(cfg), w, h, d, kind, dtype, levels, C.byref(layout))
        return err, layout

    def _mip_chain_volume_buffers(self, ctx, image, kind, levels, blocks):
        """As _mip_chain_buffers for a [Z, H, W, 4] device tensor (Z: layers or depth): level tensors are [Z_i, H_i, W_i, 4]."""
        import torch
        types = {torch.uint8: TYPE_U8, torch.float16: TYPE_F16, torch.float32: TYPE_F32}
        assert image.is_contiguous() and image.dim() == 4 and image.shape[-1] == 4, "a contiguous [Z, H, W, 4] device tensor"
        d, h, w = image.shape[0], image.shape[1], image.shape[2]
        cfg = Config()
        cfg.block_x, cfg.block_y, cfg.block_z = self._ctx_block(ctx)
        err, layout = self.mip_chain_volume_layout(cfg, w, h, d, kind, types[image.dtype], levels)
        if err:
            raise AstcError(err, "astcenc_amd_mip_chain_volume_layout")
        store = torch.empty(max(layout.texels_len, 1), dtype=torch.uint8, device=image.device)
        tensors = [image]
        for i in range(1, layout.level_count):
            size = layout.dim_x[i] * layout.dim_y[i] * layout.dim_z[i] * 4 * image.element_size()
            tensors.append(store[layout.texels_offset[i]:layout.texels_offset[i] + size].view(image.dtype)
                           .view(layout.dim_z[i], layout.dim_y[i], layout.dim_x[i], 4))
        out = torch.empty(layout.blocks_len, dtype=torch.uint8, device=image.device) if blocks else None
        return (w, h, d), types[image.dtype], layout, store, tensors, out

    def generate_mip_chain_volume_device(self, ctx, image, kind=MIP_VOLUME, levels=0, stream=None):
        """Levels of the [Z, H, W, 4] device tensor `image` (astcenc_amd_generate_mip_chain_volume_device): a list of [Z_i, H_i,
        W_i, 4] torch views, level 0 being `image` itself."""
        (w, h, d), dtype, layout, store, tensors, _ = self._mip_chain_volume_buffers(ctx, image, kind, levels, False)
        err = self.lib.astcenc_amd_generate_mip_chain_volume_device(ctx, image.data_ptr(), w, h, d, kind, dtype, layout.level_count,
                                                                    store.data_ptr(), layout.texels_len, torch_stream(stream, image.device))
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_volume_device")
        return tensors

    def compress_mip_chain_volume_device(self, ctx, image, kind=MIP_VOLUME, levels=0, swizzle=SWZ_RGBA, stream=None):
        """astcenc_amd_compress_mip_chain_volume_device: returns (level tensors, per-level block tensors); the kernel time of
        the call (ms, generation included) in self.last_kernel_ms."""
        (w, h, d), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(ctx, image, kind, levels, True)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_mip_chain_volume_device(ctx, image.data_ptr(), w, h, d, kind, dtype, C.byref(Swizzle(*swizzle)),
                                                                    layout.level_count, store.data_ptr(), layout.texels_len,
                                                                    out.data_ptr(), layout.blocks_len, torch_stream(stream, image.device), C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_compress_mip_chain_volume_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        return tensors, [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]

    @staticmethod
    def _mip_options(options):
        """A MipOptions, a (flags, alpha_cutoff) tuple or None (null options) -> the ctypes argument."""
        if options is None:
            return None
        return C.byref(options if isinstance(options, MipOptions) else MipOptions(*options))

    def generate_mip_chain_ex_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, stream=None):
        """astcenc_amd_generate_mip_chain_ex_device: generate_mip_chain_volume_device with mip options (see _mip_options)."""
        (w, h, d), dtype, layout, store, tensors, _ = self._mip_chain_volume_buffers(ctx, image, kind, levels, False)
        err = self.lib.astcenc_amd_generate_mip_chain_ex_device(ctx, image.data_ptr(), w, h, d, kind, dtype, layout.level_count,
                                                                self._mip_options(options), store.data_ptr(), layout.texels_len,
                                                                torch_stream(stream, image.device))
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_ex_device")
        return tensors

    def compress_mip_chain_ex_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, swizzle=SWZ_RGBA, stream=None):
        """astcenc_amd_compress_mip_chain_ex_device: compress_mip_chain_volume_device with mip options; returns (level tensors,
        per-level block tensors), the kernel time of the call in self.last_kernel_ms."""
        (w, h, d), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(ctx, image, kind, levels, True)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_mip_chain_ex_device(ctx, image.data_ptr(), w, h, d, kind, dtype, C.byref(Swizzle(*swizzle)),
                                                                layout.level_count, self._mip_options(options), store.data_ptr(),
                                                                layout.texels_len, out.data_ptr(), layout.blocks_len, torch_stream(stream, image.device),
                                                                C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_compress_mip_chain_ex_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        return tensors, [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]

    @staticmethod
    def _mip_filter(mip_filter):
        """A MipFilter, a (kind, edge) tuple or None (null filter: the box) -> the ctypes argument."""
        if mip_filter is None:
            return None
        return C.byref(mip_filter if isinstance(mip_filter, MipFilter) else MipFilter(*mip_filter))

    def generate_mip_chain_filtered_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, mip_filter=None, stream=None):
        """astcenc_amd_generate_mip_chain_filtered_device: generate_mip_chain_ex_device with a mip filter (see _mip_filter)."""
        (w, h, d), dtype, layout, store, tensors, _ = self._mip_chain_volume_buffers(ctx, image, kind, levels, False)
        err = self.lib.astcenc_amd_generate_mip_chain_filtered_device(ctx, image.data_ptr(), w, h, d, kind, dtype, layout.level_count,
                                                                      self._mip_options(options), self._mip_filter(mip_filter),
                                                                      store.data_ptr(), layout.texels_len, torch_stream(stream, image.device))
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_filtered_device")
        return tensors

    def compress_mip_chain_filtered_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, mip_filter=None, swizzle=SWZ_RGBA,
                                           stream=None):
        """astcenc_amd_compress_mip_chain_filtered_device: compress_mip_chain_ex_device with a mip filter; returns (level tensors,
        per-level block tensors), the kernel time of the call in self.last_kernel_ms."""
        (w, h, d), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(ctx, image, kind, levels, True)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_mip_chain_filtered_device(ctx, image.data_ptr(), w, h, d, kind, dtype, C.byref(Swizzle(*swizzle)),
                                                                      layout.level_count, self._mip_options(options),
                                                                      self._mip_filter(mip_filter), store.data_ptr(), layout.texels_len,
                                                                      out.data_ptr(), layout.blocks_len, torch_stream(stream, image.device), C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_compress_mip_chain_filtered_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        return tensors, [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]

    @staticmethod
    def _mip_weighting(weighting):
        """A MipWeighting, a MIP_WEIGHT_* value or None (null weighting: none) -> the ctypes argument."""
        if weighting is None:
            return None
        return C.byref(weighting if isinstance(weighting, MipWeighting) else MipWeighting(weighting))

    def generate_mip_chain_weighted_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, mip_filter=None, stream=None,
                                           weighting=None):
        """astcenc_amd_generate_mip_chain_weighted_device: generate_mip_chain_filtered_device with a weighting (see
        _mip_weighting)."""
        (w, h, d), dtype, layout, store, tensors, _ = self._mip_chain_volume_buffers(ctx, image, kind, levels, False)
        err = self.lib.astcenc_amd_generate_mip_chain_weighted_device(ctx, image.data_ptr(), w, h, d, kind, dtype, layout.level_count,
                                                                      self._mip_options(options), self._mip_filter(mip_filter),
                                                                      self._mip_weighting(weighting), store.data_ptr(), layout.texels_len,
                                                                      torch_stream(stream, image.device))
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_weighted_device")
        return tensors

    def compress_mip_chain_weighted_device(self, ctx, image, kind=MIP_VOLUME, levels=0, options=None, mip_filter=None, swizzle=SWZ_RGBA,
                                           stream=None, weighting=None):
        """astcenc_amd_compress_mip_chain_weighted_device: compress_mip_chain_filtered_device with a weighting; returns (level
        tensors, per-level block tensors), the kernel time of the call in self.last_kernel_ms."""
        (w, h, d), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(ctx, image, kind, levels, True)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_compress_mip_chain_weighted_device(ctx, image.data_ptr(), w, h, d, kind, dtype, C.byref(Swizzle(*swizzle)),
                                                                      layout.level_count, self._mip_options(options),
                                                                      self._mip_filter(mip_filter), self._mip_weighting(weighting),
                                                                      store.data_ptr(), layout.texels_len, out.data_ptr(), layout.blocks_len,
                                                                      torch_stream(stream, image.device), C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_compress_mip_chain_weighted_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        return tensors, [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]

    def compress_mip_chain_adaptive(self, base_ctx, strong_ctx, image, criterion, max_blocks=NO_BLOCK_BUDGET, kind=MIP_VOLUME, levels=0,
                                    options=None, mip_filter=None, weighting=None, swizzle=SWZ_RGBA, decode_swizzle=SWZ_RGBA,
                                    block_errors=None, stream=None):
        """The adaptive driver over the mip chain of the [Z, H, W, 4] device tensor `image`: the levels are generated with
        astcenc_amd_generate_mip_chain_weighted_device (base_ctx), one set entry per level is built from the layout, and
        astcenc_amd_compress_images_adaptive_device compresses the set.  Returns (level tensors, per-level block tensors,
        AdaptiveSetStats)."""
        (w, h, d), dtype, layout, store, tensors, out = self._mip_chain_volume_buffers(base_ctx, image, kind, levels, True)
        s = torch_stream(stream, image.device)
        err = self.lib.astcenc_amd_generate_mip_chain_weighted_device(base_ctx, image.data_ptr(), w, h, d, kind, dtype, layout.level_count,
                                                                      self._mip_options(options), self._mip_filter(mip_filter),
                                                                      self._mip_weighting(weighting), store.data_ptr(), layout.texels_len, s)
        if err:
            raise AstcError(err, "astcenc_amd_generate_mip_chain_weighted_device")
        n = layout.level_count
        ends = [layout.blocks_offset[i] for i in range(1, n)] + [layout.blocks_len]
        blocks = [out[layout.blocks_offset[i]:ends[i]] for i in range(n)]
        entries = [image_set_entry(tensors[i], blocks[i], swizzle) for i in range(n)]
        err, stats = self.compress_images_adaptive_device(base_ctx, strong_ctx, entries, criterion, max_blocks, decode_swizzle, block_errors, s)
        if err:
            raise AstcError(err, "astcenc_amd_compress_images_adaptive_device")
        return tensors, blocks, stats

    def resize_dims(self, w, h, max_dim=0, pow2=POW2_NONE):
        """astcenc_amd_resize_dims: returns (error, (out_w, out_h))."""
        x, y = C.c_uint(0), C.c_uint(0)
        err = self.lib.astcenc_amd_resize_dims(w, h, max_dim, pow2, C.byref(x), C.byref(y))
        return err, (x.value, y.value)

    def resize_image_device(self, ctx, image, size, kind=MIP_VOLUME, mip_filter=(MIP_FILTER_LANCZOS3, MIP_EDGE_CLAMP),
                            weighting=MIP_WEIGHT_NONE, stream=None):
        """astcenc_amd_resize_image_device: the [Z, H, W, 4] device tensor `image` resized to size = (w, h) (the depth or the
        layers kept) or (w, h, d); returns a new [d, h, w, 4] tensor, the kernel time in self.last_kernel_ms."""
        import torch
        types = {torch.uint8: TYPE_U8, torch.float16: TYPE_F16, torch.float32: TYPE_F32}
        assert image.is_contiguous() and image.dim() == 4 and image.shape[-1] == 4, "a contiguous [Z, H, W, 4] device tensor"
        d, h, w = image.shape[0], image.shape[1], image.shape[2]
        ow, oh, od = (tuple(size) + (d,))[:3]
        flt = mip_filter if isinstance(mip_filter, MipFilter) else MipFilter(*mip_filter)
        wt = weighting if isinstance(weighting, MipWeighting) else MipWeighting(weighting)
        out = torch.empty((od, oh, ow, 4), dtype=image.dtype, device=image.device)
        ms = C.c_float(0.0)
        err = self.lib.astcenc_amd_resize_image_device(ctx, image.data_ptr(), w, h, d, kind, types[image.dtype],
                                                       C.byref(Resize(ow, oh, od, flt, wt)), out.data_ptr(),
                                                       out.numel() * out.element_size(), torch_stream(stream, image.device), C.byref(ms))
        self.last_kernel_ms = ms.value
        if err:
            raise AstcError(err, "astcenc_amd_resize_image_device")
        return out

    def decompress(self, data, width, height, block=(6, 6), profile=PRF_LDR, out_type=np.uint8, depth=None):
        """Decode blocks back to [H, W, 4] ([D, H, W, 4] when depth is given) through
        astcenc_decompress_image of whichever library this is."""
        bz = block[2] if len(block) > 2 else 1
        err, cfg = self.config_init(profile, block[0], block[1], bz, PRE_MEDIUM, FLG_DECOMPRESS_ONLY)
        if err:
            raise AstcError(err, "astcenc_config_init")
        err, ctx = self.context_alloc(cfg, 1)
        if err:
            raise AstcError(err, "astcenc_context_alloc")
        try:
            d = 1 if depth is None else depth
            out = np.zeros((height, width, 4) if depth is None else (depth, height, width, 4), dtype=out_type)
            dtype = {np.dtype(np.uint8): TYPE_U8, np.dtype(np.float16): TYPE_F16, np.dtype(np.float32): TYPE_F32}[out.dtype]
            slice_bytes = height * width * 4 * out.dtype.itemsize
            slices = (C.c_void_p * d)(*[out.ctypes.data + z * slice_bytes for z in range(d)])
            img = Image(width, height, d, dtype, slices)
            swz = Swizzle(*SWZ_RGBA)
            data = np.ascontiguousarray(data, dtype=np.uint8)
            err = self.lib.astcenc_decompress_image(ctx, data.ctypes.data, data.nbytes, C.byref(img), C.byref(swz), 0)
            if err:
                raise AstcError(err, "astcenc_decompress_image")
            return out
        finally:
            self.context_free(ctx)


_SAMPLE_LOD_FUNCTION = None


def _sample_lod_function():
    """The torch.autograd.Function behind Library.sample_lod, made on first use: torch is imported lazily in this module."""
    global _SAMPLE_LOD_FUNCTION
    if _SAMPLE_LOD_FUNCTION is not None:
        return _SAMPLE_LOD_FUNCTION
    import torch
    dtypes = {TENSOR_F32: torch.float32, TENSOR_F16: torch.float16, TENSOR_BF16: torch.bfloat16}

    class SampleLod(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coords, lod, lib, ctx, entries, format, sampler, first_entry, level_count, z, lod_bias):
            coords = coords.detach().contiguous()
            lod = lod.detach().contiguous() if lod is not None else None
            h, w = coords.shape[0], coords.shape[1]
            shape = (format.channels, h, w) if format.layout == TENSOR_PLANAR else (h, w, format.channels)
            out = torch.empty(shape, dtype=dtypes[format.type], device=coords.device)
            err = lib.sample_lod_tensors_device(ctx, entries, format, sampler, [(first_entry, level_count, z, coords, lod, out, lod_bias)])
            if err != SUCCESS:
                raise AstcError(err, "astcenc_amd_sample_lod_tensors_device")
            fctx.save_for_backward(coords, *([lod] if lod is not None else []))
            fctx.call = (lib, ctx, entries, format, sampler, first_entry, level_count, z, lod_bias)
            return out

        @staticmethod
        def backward(fctx, grad_out):
            lib, ctx, entries, format, sampler, first_entry, level_count, z, lod_bias = fctx.call
            saved = fctx.saved_tensors
            coords, lod = saved[0], saved[1] if len(saved) > 1 else None
            grad_out = grad_out.contiguous()
            grad_coords = torch.empty_like(coords)
            grad_lod = torch.empty_like(lod) if lod is not None and fctx.needs_input_grad[1] else None
            err = lib.sample_lod_grad_device(ctx, entries, format, sampler, [(first_entry, level_count, z, coords, lod, grad_out, grad_coords, grad_lod, lod_bias)])
            if err != SUCCESS:
                raise AstcError(err, "astcenc_amd_sample_lod_grad_device")
            return (grad_coords, grad_lod) + (None,) * 9

    _SAMPLE_LOD_FUNCTION = SampleLod
    return SampleLod


_SAMPLE_VOLUME_FUNCTION = None


def _sample_volume_function():
    """The torch.autograd.Function behind Library.sample_volume, made on first use like _sample_lod_function."""
    global _SAMPLE_VOLUME_FUNCTION
    if _SAMPLE_VOLUME_FUNCTION is not None:
        return _SAMPLE_VOLUME_FUNCTION
    import torch
    dtypes = {TENSOR_F32: torch.float32, TENSOR_F16: torch.float16, TENSOR_BF16: torch.bfloat16}

    class SampleVolume(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coords, lod, lib, ctx, entries, format, sampler, first_entry, level_count, lod_bias):
            coords = coords.detach().contiguous()
            lod = lod.detach().contiguous() if lod is not None else None
            h, w = coords.shape[0], coords.shape[1]
            shape = (format.channels, h, w) if format.layout == TENSOR_PLANAR else (h, w, format.channels)
            out = torch.empty(shape, dtype=dtypes[format.type], device=coords.device)
            err = lib.sample_volume_tensors_device(ctx, entries, format, sampler, [(first_entry, level_count, coords, lod, out, lod_bias)])
            if err != SUCCESS:
                raise AstcError(err, "astcenc_amd_sample_volume_tensors_device")
            fctx.save_for_backward(coords, *([lod] if lod is not None else []))
            fctx.call = (lib, ctx, entries, format, sampler, first_entry, level_count, lod_bias)
            return out

        @staticmethod
        def backward(fctx, grad_out):
            lib, ctx, entries, format, sampler, first_entry, level_count, lod_bias = fctx.call
            saved = fctx.saved_tensors
            coords, lod = saved[0], saved[1] if len(saved) > 1 else None
            grad_out = grad_out.contiguous()
            grad_coords = torch.empty_like(coords)
            grad_lod = torch.empty_like(lod) if lod is not None and fctx.needs_input_grad[1] else None
            err = lib.sample_volume_grad(ctx, entries, format, sampler, [(first_entry, level_count, coords, lod, grad_out, grad_coords, grad_lod, lod_bias)])
            if err != SUCCESS:
                raise AstcError(err, "astcenc_amd_sample_volume_grad_device")
            return (grad_coords, grad_lod) + (None,) * 8

    _SAMPLE_VOLUME_FUNCTION = SampleVolume
    return SampleVolume


def torch_stream(stream=None, device=None):
    """The hip_stream argument of a device call: the raw hipStream_t of a torch stream, a raw handle as it is, or that of
    torch's current stream on `device` (None: torch's current device) for None.  Handle 0 is torch's default stream, the legacy
    null stream, but a NULL hip_stream is the context's own non-blocking stream (include/astcenc_amd.h), which waits for nothing
    queued on the null stream: the default stream of `device` is synchronised here first, so that what torch queued before the
    call -- the call's inputs, fills of its outputs -- is done when the call starts.  Every call synchronises its stream before it
    returns, so the host would have waited for that work either way."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    handle = getattr(stream, "cuda_stream", stream)
    if not handle:
        import torch
        torch.cuda.default_stream(getattr(stream, "device", device)).synchronize()
    return handle


def synthetic_image(width, height, seed=0x9E3779B1):
    """Deterministic integer-only RGBA8 test image: smooth ramps, a 32x32 checker of
    hard edges on R, and per-channel hash noise.  No libm, so every host produces identical bytes."""
    y, x = np.meshgrid(np.arange(height, dtype=np.int64), np.arange(width, dtype=np.int64), indexing="ij")

    def tri(v):
        m = v & 511
        return np.where(m < 256, m, 511 - m)

    r = (3 * tri(x + 2 * y) + tri((3 * x - y) >> 1)) >> 2
    checker = ((x >> 5) + (y >> 5)) & 1
    r = np.where(checker == 1, 255 - r, r)
    g = (3 * tri(2 * x - y + 128) + tri((x + 3 * y) >> 2)) >> 2
    b = 255 - ((tri(x + y) + tri((x - y) >> 1)) >> 1)
    a = 192 + (tri((x >> 1) + (y >> 2)) >> 2)

    def noise(c, amp):
        h = (x * 0x85EBCA6B + y * 0xC2B2AE35 + c * 0x27D4EB2F + seed) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
        h ^= h >> 12
        h = (h * 0x297A2D39) & 0xFFFFFFFF
        h ^= h >> 15
        return (h % (2 * amp + 1)) - amp

    out = np.stack([r + noise(0, 10), g + noise(1, 10), b + noise(2, 10), a + noise(3, 3)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def synthetic_hdr_image(width, height, seed=0x9E3779B1):
    """HDR companion of synthetic_image: the LDR generator / 255 with RGB scaled by
    2^(-2..5) in 8x8 patches (exponent ((tri(x >> 3) + tri(y >> 3)) >> 6) - 2), alpha kept in 0..1, stored as
    RGBA16F (round to nearest even).  Power-of-two scaling of exact quotients: identical bytes on every host."""
    base = synthetic_image(width, height, seed).astype(np.float32) / np.float32(255.0)
    y, x = np.meshgrid(np.arange(height, dtype=np.int64), np.arange(width, dtype=np.int64), indexing="ij")

    def tri(v):
        m = v & 511
        return np.where(m < 256, m, 511 - m)

    expo = ((tri(x >> 3) + tri(y >> 3)) >> 6) - 2
    scale = np.ldexp(np.float32(1.0), expo.astype(np.int32)).astype(np.float32)
    base[..., :3] *= scale[..., None]
    return base.astype(np.float16)


def psnr_rgba8(a, b):
    """10*log10(samples / sum((a-b)^2)) on values/255, double accumulation (ref: astcenccli_error_metrics.cpp:240-346)."""
    d = (a.astype(np.float64) - b.astype(np.float64)) / 255.0
    s = float((d * d).sum())
    return float("inf") if s == 0 else 10.0 * np.log10(a.size / s)


# ---- multi-GPU sharding: contiguous block rows per rank, no data-path collective ----

def block_row_shard(dim_y, block_y, rank, world):
    """Rows of blocks [row0, row1) owned by `rank`, and the texel rows [y0, y1) that feed them.

    Blocks are independent (ref: astcenc_entry.cpp:1009-1038: compress_block reads only its own
    texels and writes its own 16 bytes), so a shard is just a sub-image whose top edge sits on a block
    boundary; only the last shard can contain a partial (edge-clamped) block row.  Ranks beyond the
    number of block rows get an empty shard.
    """
    blocks_y = (dim_y + block_y - 1) // block_y
    per = (blocks_y + world - 1) // world
    row0 = min(rank * per, blocks_y)
    row1 = min(row0 + per, blocks_y)
    return row0, row1, min(row0 * block_y, dim_y), min(row1 * block_y, dim_y)


def compress_shard(lib, ctx, pixels, block, rank, world, out=None):
    """Compress this rank's block rows of `pixels` ([H, W, 4]) with context `ctx`.

    Returns (byte offset into the whole image's block stream, uint8 blocks of the shard).  When
    `out` (the whole image's output array) is given, the shard is also written in place.
    """
    h, w = pixels.shape[0], pixels.shape[1]
    row0, row1, y0, y1 = block_row_shard(h, block[1], rank, world)
    blocks_x = (w + block[0] - 1) // block[0]
    offset = row0 * blocks_x * 16
    part = np.zeros((row1 - row0) * blocks_x * 16, dtype=np.uint8)
    if row1 > row0:
        err = lib.compress_raw(ctx, np.ascontiguousarray(pixels[y0:y1]), part)
        if err:
            raise AstcError(err, "astcenc_compress_image (shard %d/%d)" % (rank, world))
    if out is not None:
        out[offset: offset + part.size] = part
    return offset, part


# ---- .astc container (ref: Docs/FileFormat.md, astcenccli_image_load_store.cpp: 16-byte header) ----

ASTC_MAGIC = bytes([0x13, 0xAB, 0xA1, 0x5C])


def write_astc(path, blocks, width, height, block, depth=1):
    """Write a block stream as an .astc file: magic, block dims (3 x u8), image dims (3 x 24-bit LE), data."""
    def u24(v):
        return bytes([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF])
    bz = block[2] if len(block) > 2 else 1
    header = ASTC_MAGIC + bytes([block[0], block[1], bz]) + u24(width) + u24(height) + u24(depth)
    data = np.ascontiguousarray(blocks, dtype=np.uint8).tobytes()
    with open(path, "wb") as f:
        f.write(header + data)


def read_astc(path):
    """-> (blocks uint8[n*16], width, height, depth, (bx, by, bz)); raises ValueError on a malformed file
    (bad magic, zero dimensions, truncated payload), like the reference loader."""
    raw = open(path, "rb").read()
    if len(raw) < 16 or raw[:4] != ASTC_MAGIC:
        raise ValueError("not an .astc file")
    bx, by, bz = raw[4], raw[5], raw[6]
    dims = [raw[7 + 3 * i] | (raw[8 + 3 * i] << 8) | (raw[9 + 3 * i] << 16) for i in range(3)]
    if 0 in (bx, by, bz) or 0 in dims:
        raise ValueError("zero dimension in .astc header")
    n = ((dims[0] + bx - 1) // bx) * ((dims[1] + by - 1) // by) * ((dims[2] + bz - 1) // bz)
    if len(raw) - 16 < n * 16:
        raise ValueError("truncated .astc payload")
    return np.frombuffer(raw, dtype=np.uint8, count=n * 16, offset=16).copy(), dims[0], dims[1], dims[2], (bx, by, bz)


# ---- KTX 1.1 container for compressed data (ref: store_ktx_compressed_image / load_ktx_compressed_image,
# astcenccli_image_load_store.cpp:1294-1437; GL enums :725-775) ----

KTX_MAGIC = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
GL_RGBA = 0x1908
_KTX_2D = [(4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12)]
_KTX_3D = [(3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4), (5, 4, 4), (5, 5, 4), (5, 5, 5), (6, 5, 5), (6, 6, 5), (6, 6, 6)]


def ktx_gl_format(block, srgb=False):
    """glInternalFormat of an ASTC footprint: COMPRESSED_RGBA_ASTC_* / COMPRESSED_SRGB8_ALPHA8_ASTC_* (+ _OES for 3D)."""
    bz = block[2] if len(block) > 2 else 1
    if bz <= 1:
        return (0x93D0 if srgb else 0x93B0) + _KTX_2D.index((block[0], block[1]))
    return (0x93E0 if srgb else 0x93C0) + _KTX_3D.index((block[0], block[1], bz))


def write_ktx(path, blocks, width, height, block, depth=1, srgb=False):
    """Write a block stream as a single-level KTX 1.1 file, little endian, no key/value data."""
    import struct
    data = np.ascontiguousarray(blocks, dtype=np.uint8).tobytes()
    header = KTX_MAGIC + struct.pack("<13I", 0x04030201, 0, 1, 0, ktx_gl_format(block, srgb), GL_RGBA,
                                     width, height, 0 if depth == 1 else depth, 0, 1, 1, 0)
    with open(path, "wb") as f:
        f.write(header + struct.pack("<I", len(data)) + data)


def read_ktx(path):
    """-> (blocks uint8[], width, height, depth, (bx, by, bz), is_srgb); either byte order; raises ValueError
    on anything that is not a compressed ASTC KTX file, like the reference loader."""
    import struct
    raw = open(path, "rb").read()
    if len(raw) < 68 or raw[:12] != KTX_MAGIC:
        raise ValueError("not a KTX file")
    endian = struct.unpack_from("<I", raw, 12)[0]
    if endian not in (0x04030201, 0x01020304):
        raise ValueError("corrupt KTX header")
    e = "<" if endian == 0x04030201 else ">"
    (gl_type, type_size, gl_format, internal, base, w, h, d, _arrays, _faces, _mips, kv) = struct.unpack_from(e + "12I", raw, 16)
    if gl_type != 0 or gl_format != 0 or type_size != 1 or base != GL_RGBA:
        raise ValueError("unsupported KTX format")
    for first, table, srgb in ((0x93B0, _KTX_2D, False), (0x93D0, _KTX_2D, True), (0x93C0, _KTX_3D, False), (0x93E0, _KTX_3D, True)):
        if first <= internal < first + len(table):
            blk = table[internal - first]
            break
    else:
        raise ValueError("unsupported KTX format")
    at = 64 + kv
    if len(raw) < at + 4:
        raise ValueError("truncated KTX file")
    n = struct.unpack_from(e + "I", raw, at)[0]
    if len(raw) < at + 4 + n:
        raise ValueError("truncated KTX file")
    block = (blk[0], blk[1], blk[2] if len(blk) > 2 else 1)
    return np.frombuffer(raw, dtype=np.uint8, count=n, offset=at + 4).copy(), w, h, d if d else 1, block, srgb


def write_ktx_mips(path, level_blocks, width, height, block, srgb=False):
    """Write the blocks of a mip chain (level_blocks[i]: level i, max(1, width >> i) x max(1, height >> i) texels) as one KTX 1.1
    file: write_ktx_chain of one 2D image (depth 1, no array, one face), so a level of the wrong size is a ValueError."""
    if len(block) > 2 and block[2] > 1:
        raise ValueError("mip chains are 2D: a 2D footprint")
    write_ktx_chain(path, level_blocks, width, height, block, depth=1, layers=0, faces=1, srgb=srgb)


def read_ktx_mips(path):
    """-> ([blocks uint8[] per level], width, height, (bx, by, bz), is_srgb) of a 2D KTX 1.1 file with any number of mip levels
    (either byte order): read_ktx_chain's levels; the level sizes are checked against the footprint."""
    k = read_ktx_chain(path)
    if k["depth"] != 1 or k["layers"] != 0 or k["faces"] != 1:
        raise ValueError("not a 2D KTX file")
    return k["levels"], k["w"], k["h"], k["block"], k["srgb"]


def _ktx_chain_level_bytes(w, h, depth, layers, faces, block, i):
    """Bytes of level i of a KTX chain: every array element, face and z slice of it (a 3D footprint: its block layers)."""
    bz = block[2] if len(block) > 2 else 1
    lw, lh, ld = max(1, w >> i), max(1, h >> i), max(1, depth >> i)
    return -(-lw // block[0]) * -(-lh // block[1]) * -(-ld // bz) * 16 * max(layers, 1) * faces


def write_ktx_chain(path, level_blocks, w, h, block, depth=1, layers=0, faces=1, srgb=False):
    """Write the blocks of a mip chain of an array, a cube map (faces=6), a cube-map array or a volume (depth > 1, a 3D
    footprint) as one KTX 1.1 file.  level_blocks[i] holds level i in KTX order: array elements, then faces, then z slices --
    the order of the layers of an ASTCENC_AMD_MIP_ARRAY chain (a cube map's layers face-major within each element).
    imageSize is the whole level, except for a cube map that is not an array, where it is one face.  ASTC data is whole
    16-byte blocks, so there is no cube or mip padding."""
    import struct
    bz = block[2] if len(block) > 2 else 1
    if faces not in (1, 6):
        raise ValueError("faces must be 1 or 6")
    if depth > 1 and bz <= 1:
        raise ValueError("a volume needs a 3D footprint: KTX has no 2D-ASTC volume format")
    if faces == 6 and (w != h or depth > 1):
        raise ValueError("cube map faces must be square and 2D")
    if depth > 1 and layers:
        raise ValueError("arrays of volumes are not supported")
    header = KTX_MAGIC + struct.pack("<13I", 0x04030201, 0, 1, 0, ktx_gl_format(block, srgb), GL_RGBA,
                                     w, h, 0 if depth <= 1 else depth, layers, faces, len(level_blocks), 0)
    with open(path, "wb") as f:
        f.write(header)
        for i, blocks in enumerate(level_blocks):
            data = np.ascontiguousarray(blocks if isinstance(blocks, np.ndarray) else blocks.cpu().numpy(), dtype=np.uint8).tobytes()
            if len(data) != _ktx_chain_level_bytes(w, h, depth, layers, faces, block, i):
                raise ValueError("level %d holds %d bytes, its size is %d" % (i, len(data), _ktx_chain_level_bytes(w, h, depth, layers, faces, block, i)))
            cube = faces == 6 and layers == 0
            f.write(struct.pack("<I", len(data) // 6 if cube else len(data)) + data)


def read_ktx_chain(path):
    """-> {"levels": [blocks uint8[] per level, KTX order], "w", "h", "depth", "layers", "faces", "block": (bx, by, bz), "srgb"}
    of a KTX 1.1 file with any number of mip levels, array elements and faces (either byte order); every imageSize is checked
    against the level's size."""
    import struct
    raw = open(path, "rb").read()
    _, w, h, depth, block, srgb = read_ktx(path)
    e = "<" if struct.unpack_from("<I", raw, 12)[0] == 0x04030201 else ">"
    layers, faces, mips, kv = struct.unpack_from(e + "4I", raw, 48)
    if faces not in (1, 6):
        raise ValueError("bad KTX face count")
    at, levels = 64 + kv, []
    cube = faces == 6 and layers == 0
    for i in range(max(mips, 1)):
        size = _ktx_chain_level_bytes(w, h, depth, layers, faces, block, i)
        if len(raw) < at + 4:
            raise ValueError("truncated KTX file")
        n = struct.unpack_from(e + "I", raw, at)[0]
        if n != (size // 6 if cube else size) or len(raw) < at + 4 + size:
            raise ValueError("bad KTX mip level %d" % i)
        levels.append(np.frombuffer(raw, dtype=np.uint8, count=size, offset=at + 4).copy())
        at += 4 + size
    return {"levels": levels, "w": w, "h": h, "depth": depth, "layers": layers, "faces": faces, "block": block, "srgb": srgb}
