/* SPDX-License-Identifier: Apache-2.0
 *
 * astcenc_amd.h -- MI355X-specific additions to the astcenc C ABI (libastcenc_amd.so).
 *
 * The reference API (include/astcenc.h) takes host pointers, so every astcenc_compress_image()
 * pays a PCIe round trip.  Pipelines that already hold their textures in HBM (and the benchmark,
 * which must time the kernels with inputs resident) use the entry point below instead.  It runs
 * the same kernels with the same context; nothing else about the contract changes.
 */
#ifndef ASTCENC_AMD_INCLUDED
#define ASTCENC_AMD_INCLUDED

#include "astcenc.h"

/* Compress a 2D image that is already resident in device memory.
 *
 *   device_image : device pointer, tightly packed RGBA rows, dim_x * dim_y texels of data_type
 *   device_out   : device pointer, receives 16 bytes per block in raster block order
 *   data_len     : bytes available at device_out (>= 16 * blocks, else ASTCENC_ERR_OUT_OF_MEM)
 *   hip_stream   : hipStream_t to launch on (NULL = the context's own stream); the call returns
 *                  after the work on that stream has completed.  The context's own stream is a
 *                  non-blocking stream (hipStreamNonBlocking), NOT the legacy null stream: work
 *                  queued on the null stream -- a kernel that produces device_image, a fill of
 *                  device_out -- is not waited for.  A caller whose work is on the null stream
 *                  synchronises it before the call.  This holds for every hip_stream below.
 *   kernel_ms    : optional; receives the elapsed time of the compression kernel(s) measured with
 *                  HIP events recorded on that stream around the launches
 *
 * Same argument checks and error codes as astcenc_compress_image (ref: Source/astcenc_entry.cpp:1134-1182).
 * Single caller per context (no thread_index rendezvous). */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_image_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	void* device_out, size_t data_len,
	void* hip_stream,
	float* kernel_ms);

/* The same for a volume or 2D array image: dim_z slices of dim_x * dim_y texels back to back at
 * device_volume, compressed with the context's 2D or 3D footprint into blocks in x, y, z raster order
 * (ref: the z loop of compress_image, Source/astcenc_entry.cpp:961-966, and astcenc_image::data[z]).
 * Every slice is compressed from its own data (see ASTCENC_AMD_OPT_PER_SLICE_FAST_LOAD below for the one case in
 * which astcenc_compress_image deliberately does not).
 * The context's progress_callback, if any, is called from the calling thread here; astcenc_compress_image on a
 * context that shards over several devices (ASTCENC_AMD_DEVICES) calls it from library-created threads as well,
 * serialised, with a monotonic percentage. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_volume_device(
	struct astcenc_context* context,
	const void* device_volume,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	void* device_out, size_t data_len,
	void* hip_stream,
	float* kernel_ms);

/* Decompress blocks that are resident in device memory into a device image (dim_z slices of tightly
 * packed RGBA rows of data_type, back to back).  Same checks, profiles, output types and swizzles as
 * astcenc_decompress_image (ref: Source/astcenc_entry.cpp:1274-1390); returns when the work on
 * hip_stream (NULL = the context's own stream) has completed. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_decompress_image_device(
	struct astcenc_context* context,
	const void* device_blocks, size_t data_len,
	void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	void* hip_stream);

/* Image sets: many device-resident images -- a mip chain, the textures of a scene, a batch of a dataset -- compressed or
 * decompressed in one call with one context.  One entry per image.  Compression reads `image` and writes `blocks`;
 * decompression reads `blocks` and writes `image`, so one array can describe both directions. */
struct astcenc_amd_image_set_entry {
	void* image;                   /* device pointer: dim_z slices of dim_x * dim_y texels, tightly packed RGBA rows */
	void* blocks;                  /* device pointer: 16 bytes per block, raster block order */
	size_t blocks_len;             /* bytes available at / readable from `blocks` */
	unsigned int dim_x, dim_y, dim_z;
	enum astcenc_type data_type;
	struct astcenc_swizzle swizzle;
};

/* Compress every entry of entries[0 .. entry_count).  Every entry's blocks are exactly those astcenc_amd_compress_volume_device
 * writes for that entry alone -- its per-slice loading default and ASTCENC_AMD_OPT_PER_SLICE_FAST_LOAD, the alpha-scale pre-pass
 * (run per entry, 2D footprints), the entry's own data type and swizzle -- but the blocks of all entries run in the same chain
 * of kernel launches, so that a set of small images fills the device as one large image does.
 *
 *   - Every entry is checked with the checks and error codes of astcenc_amd_compress_volume_device (a null `image` or `blocks`:
 *     ASTCENC_ERR_BAD_CONTEXT, as there), all of them before anything is launched: a bad entry makes the call return its error
 *     with nothing written, and the log callback (astcenc_amd_set_log_callback) names the entry's index.
 *   - entry_count == 0 returns ASTCENC_SUCCESS and does nothing; a null `entries` with a non-zero count, a null context, or a
 *     set of more than 2^32 - 1 blocks in all return ASTCENC_ERR_BAD_PARAM.
 *   - The call runs on the device that owns entry 0's image; a buffer of any entry on another device returns
 *     ASTCENC_ERR_BAD_PARAM.  Outputs must not overlap each other or any input (not checked).
 *   - Cancel, progress and timing as in astcenc_amd_compress_volume_device: the same cancel rules; the progress callback sees a
 *     monotonic percentage of the whole set's blocks; kernel_ms covers every launch of the call; the call returns once the
 *     work on hip_stream has completed. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_images_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	void* hip_stream, float* kernel_ms);

/* Decompress every entry: each entry's image is exactly what astcenc_amd_decompress_image_device writes for that entry alone
 * (same checks and error codes, all before anything is launched), one launch for the whole set.  Same argument rules as above. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_decompress_images_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	void* hip_stream);

/* Decoding parts of compressed images: many rectangles (boxes) of many compressed images in one launch -- a batch of crops, a
 * tile of a mip level, the neighbourhood of a block -- each into a caller buffer with its own origin and pitches.  Only the
 * blocks a window covers are read and decoded; nothing the size of a source image is written or allocated.
 *
 * A region names a window of one entry and where it goes. */
struct astcenc_amd_decode_region {
	unsigned int entry;                     /* index into entries[]: the compressed image the window lies in */
	unsigned int x, y, z;                   /* origin of the window in that image, texels */
	unsigned int size_x, size_y, size_z;    /* its size, each >= 1 */
	void* out;                              /* device pointer: size_z slices of size_y rows of size_x RGBA texels of the entry's data_type */
	size_t row_pitch, slice_pitch;          /* bytes from row to row / slice to slice of `out`; 0 = tightly packed */
};

/* Decode regions[0 .. region_count).  Texel (i, j, k) of a region's `out` is bit for bit texel (x + i, y + j, z + k) of what
 * astcenc_amd_decompress_image_device writes for that entry alone: the entry's data_type and swizzle (the Z swizzle included),
 * the context's profile, error blocks and constant-colour blocks, 2D footprints (z selects array slices) and 3D ones.  No byte
 * of `out` outside the window's texels is written: not the padding of a pitch, not what lies between regions written into one
 * atlas or batch tensor.
 *
 *   - Each entry describes a compressed image as in astcenc_amd_decompress_images_device; `image` is ignored and may be null.
 *     `blocks`, `blocks_len`, the dimensions and the swizzle of every entry get the checks and error codes of that call.  Many
 *     regions may name one entry; an entry that no region names costs nothing.
 *   - Everything is checked before anything is launched: a failure returns its error with nothing written, and the log callback
 *     (astcenc_amd_set_log_callback) names the index of the region or entry.
 *   - region_count == 0 returns ASTCENC_SUCCESS and does nothing.  ASTCENC_ERR_BAD_PARAM: a null context; a null `regions`; a
 *     null `entries` with a non-zero entry_count; a region whose `entry` is not below entry_count, with a zero size, or whose
 *     window is not wholly inside the entry's image (x + size_x is compared in 64 bits); a non-zero pitch smaller than the tight
 *     one (size_x texels / size_y rows of row_pitch) or not a multiple of the texel size (4 / 8 / 16 bytes for U8 / F16 / F32);
 *     an `out` not aligned to the texel size; more than 2^32 - 1 work items (runs of up to 32 covered blocks of one block row) in
 *     all.  A null `out`: ASTCENC_ERR_BAD_CONTEXT, as a null buffer elsewhere.
 *   - The call runs on the device that owns entry 0's blocks; the blocks of an entry some region names or a region's `out` on
 *     another device return ASTCENC_ERR_BAD_PARAM.  Outputs must not overlap each other or any input (not checked).
 *   - The call returns once the work on hip_stream (null: the context's own stream) has completed. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_decompress_regions_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_decode_region* regions, unsigned int region_count,
	void* hip_stream);

/* Windows decoded straight into tensors: what astcenc_amd_decompress_regions_device decodes, converted, scaled, mirrored and
 * laid out the way a training step computes on it -- a batch of crops as [N, 3, H, W] halves with mean and deviation folded in,
 * every other sample mirrored -- in the same single launch, with no RGBA image in between.
 *
 * The format holds for the whole call. */
enum astcenc_amd_tensor_type {
	ASTCENC_AMD_TENSOR_F32 = 0,             /* IEEE binary32, 4 bytes an element */
	ASTCENC_AMD_TENSOR_F16 = 1,             /* IEEE binary16, 2 bytes */
	ASTCENC_AMD_TENSOR_BF16 = 2             /* bfloat16 (the upper half of a binary32), 2 bytes */
};
enum astcenc_amd_tensor_layout {
	ASTCENC_AMD_TENSOR_PLANAR = 0,          /* C, D, H, W: a plane per channel */
	ASTCENC_AMD_TENSOR_INTERLEAVED = 1      /* D, H, W, C: the channels of a texel side by side */
};
#define ASTCENC_AMD_TENSOR_FLIP_X 0x1u      /* the window's columns are written right to left */
#define ASTCENC_AMD_TENSOR_FLIP_Y 0x2u      /* ... its rows bottom to top */

struct astcenc_amd_tensor_format {
	enum astcenc_amd_tensor_type type;
	enum astcenc_amd_tensor_layout layout;
	unsigned int channels;                  /* 1..4: components 0 .. channels - 1 of the swizzled texel become channels */
	float scale[4], bias[4];                /* per output channel; the first `channels` of each are used and must be finite */
};

/* A region names a window of one entry and where it goes. */
struct astcenc_amd_tensor_region {
	unsigned int entry;                     /* index into entries[] */
	unsigned int x, y, z;                   /* origin of the window in that image, texels */
	unsigned int size_x, size_y, size_z;    /* its size, each >= 1 */
	unsigned int flags;                     /* ASTCENC_AMD_TENSOR_FLIP_X | ASTCENC_AMD_TENSOR_FLIP_Y */
	void* out;                              /* device pointer: element (c = 0, k = 0, j = 0, i = 0) */
	size_t row_pitch, slice_pitch, plane_pitch;   /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Decode regions[0 .. region_count) into tensors.  For position (i, j, k) of a region's window, 0 <= i < size_x, 0 <= j <
 * size_y, 0 <= k < size_z, and channel c < format->channels:
 *
 *   Source.  s[0 .. 3] is the texel astcenc_amd_decompress_regions_device writes for that position of that entry: the entry's
 *     data_type and swizzle (the Z swizzle and the constants 0 / 1 included), the context's profile, error blocks and
 *     constant-colour blocks as there.  s[c] is converted to binary32 exactly: a U8 code v is (float)v, 0 .. 255 -- it is not
 *     divided by 255, fold 1 / 255 into `scale`; an F16 value is widened; an F32 value is itself.  Entries of different data
 *     types may share a call.
 *   Arithmetic.  t = s[c] * scale[c] rounded to binary32, then y = t + bias[c] rounded to binary32: two IEEE operations, round
 *     to nearest even, never fused, subnormal operands and results kept.  y is stored as the format's type: F32 as it is; F16
 *     and BF16 rounded to nearest even, overflow to infinity, subnormals produced.  A NaN y of any sign and payload is stored
 *     as the type's canonical quiet NaN: 0x7FC00000, 0x7E00, 0x7FC0.
 *   Placement.  With i' = size_x - 1 - i under ASTCENC_AMD_TENSOR_FLIP_X and i otherwise, j' = size_y - 1 - j under
 *     ASTCENC_AMD_TENSOR_FLIP_Y and j otherwise (z is never mirrored), the value is element
 *       PLANAR:       c * plane_pitch + k * slice_pitch + j' * row_pitch + i'
 *       INTERLEAVED:  k * slice_pitch + j' * row_pitch + i' * channels + c
 *     of `out`, counted in elements of the format's type.  A zero pitch is the tight one: row_pitch = size_x (PLANAR) or
 *     size_x * channels (INTERLEAVED); slice_pitch = row_pitch * size_y; plane_pitch = slice_pitch * size_z (PLANAR only).
 *     No other element is written: not the padding of a pitch, not the unused channels of a wider tensor, not what lies
 *     between the regions of one batch tensor.
 *
 *   - Entries, windows, the work-item bound, device ownership, the null / zero-count cases and the stream are those of
 *     astcenc_amd_decompress_regions_device, with its error codes; everything is checked before anything is launched, a
 *     failure returns its error with nothing written, and the log callback names the index of the region or entry.
 *   - Also ASTCENC_ERR_BAD_PARAM: a null `format`; a type or layout that is not one of the above; `channels` outside 1..4; a
 *     scale or bias among the first `channels` that is not finite; flag bits other than the two above; a non-zero pitch
 *     below the tight one (formed and compared in 64 bits; a tensor extent that overflows them is an error); a non-zero
 *     plane_pitch with INTERLEAVED; an `out` not aligned to the element size.  A null `out`: ASTCENC_ERR_BAD_CONTEXT. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_decompress_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_tensor_region* regions, unsigned int region_count,
	void* hip_stream);

/* Scaled windows decoded straight into tensors: the random resized crop of a vision loader.  Every region takes a window of
 * its own size and aspect ratio and resamples it to an output size of its own -- for a batch, one fixed size -- in the same
 * single launch that decodes, normalises, mirrors and lays out; no image at the window's size exists in between.
 *
 * The filter holds for the whole call.  Both filters have taps that are exact rationals of three integers. */
enum astcenc_amd_window_filter {
	ASTCENC_AMD_WINDOW_BILINEAR = 0,        /* two taps an axis, half-texel centres */
	ASTCENC_AMD_WINDOW_BOX = 1              /* exact area average */
};

struct astcenc_amd_scaled_region {
	unsigned int entry;                     /* index into entries[] */
	unsigned int x, y, z;                   /* origin of the window in that image, texels; z: the slice */
	unsigned int size_x, size_y;            /* the window, each 1 .. 65535 */
	unsigned int out_x, out_y;              /* what it becomes, each 1 .. 65535 */
	unsigned int flags;                     /* ASTCENC_AMD_TENSOR_FLIP_X | ASTCENC_AMD_TENSOR_FLIP_Y */
	void* out;                              /* device pointer: element (c = 0, j = 0, i = 0) */
	size_t row_pitch, plane_pitch;          /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Decode and resample regions[0 .. region_count) into tensors of `format` (astcenc_amd_decompress_tensors_device's: type,
 * layout, channels, scale, bias).  For output position (i, j) of a region, 0 <= i < out_x, 0 <= j < out_y, and channel
 * c < format->channels:
 *
 *   Taps.  Along each axis on its own, with S the window's size, D the output size and p the output position (i along x, j
 *     along y), in integer arithmetic of 64 bits:
 *       BILINEAR: n = (2p + 1) * S - D (signed); i0 = floor(n / 2D), f = n - i0 * 2D, so 0 <= f < 2D.  Tap 0 is source index
 *         clamp(i0, 0, S - 1) with weight 2D - f; tap 1 is source index clamp(i0 + 1, 0, S - 1) with weight f; den = 2D.
 *         Indices are counted from the window's origin and clamp at the WINDOW's edges, not the image's: the result is that
 *         of cropping, then resizing.
 *       BOX: a = p * S, b = (p + 1) * S; the taps are the source indices k = a / D .. (b - 1) / D (integer divisions), tap k
 *         has weight min(b, (k + 1) * D) - max(a, k * D), which is at least 1; den = S.
 *     A tap of weight 0 (BILINEAR's tap 1 when f = 0) is not part of any sum and its texel is not read into one: a NaN or an
 *     infinity there does not reach the result.  (BILINEAR, S = 2, D = 3: texel 0, (t0 + t1) / 2, texel 1.  BOX, S = 3, D = 2:
 *     (2 t0 + t1) / 3, (t1 + 2 t2) / 3.)
 *   Source.  v(kx, ky)[c] is component c of the texel astcenc_amd_decompress_regions_device writes for position (kx, ky) of
 *     the window at slice z: the entry's data_type and swizzle, the context's profile, error blocks and constant-colour blocks
 *     as there.  The filter works on those stored values as they are: no sRGB linearisation and no alpha weighting is done.
 *     Entries of different data types may share a call.
 *       v is widened to binary64 (exact for U8 codes 0 .. 255, F16 and F32 values).  Per source row ky that has a y tap:
 *         r(ky) = sum over the x taps, in increasing tap order, of (double)wx * v(kx, ky)[c];
 *       then acc = sum over the y taps, in increasing tap order, of (double)wy * r(ky).  A sum starts as its first product
 *       (nothing is added to a zero); every product and every sum is one IEEE binary64 operation, round to nearest even,
 *       never fused.  s[c] = (float)(acc / ((double)den_x * (double)den_y)): one binary64 division, one rounding to binary32.
 *       For U8 entries every product and sum is an integer below 2^42, exact in binary64: acc is the integer
 *       N = sum wy * (sum wx * v), and s[c] is N / (den_x * den_y) correctly rounded to binary64, then to binary32.
 *   Arithmetic, storage.  Those of astcenc_amd_decompress_tensors_device: t = s[c] * scale[c], y = t + bias[c], two binary32
 *     roundings; F32 / F16 / BF16 round to nearest even; a NaN y is stored as the type's canonical quiet NaN.
 *   Placement.  The flips apply to the OUTPUT position: i' = out_x - 1 - i under ASTCENC_AMD_TENSOR_FLIP_X and i otherwise,
 *     j' = out_y - 1 - j under ASTCENC_AMD_TENSOR_FLIP_Y and j otherwise; the value is element
 *       PLANAR:       c * plane_pitch + j' * row_pitch + i'
 *       INTERLEAVED:  j' * row_pitch + i' * channels + c
 *     of `out`.  A zero pitch is the tight one: row_pitch = out_x (PLANAR) or out_x * channels (INTERLEAVED); plane_pitch =
 *     row_pitch * out_y (PLANAR only).  No other element is written.
 *
 *   Consequence: with out_x = size_x and out_y = size_y either filter writes bit for bit what
 *   astcenc_amd_decompress_tensors_device writes for the same window (size_z = 1): every position has one tap of weight den
 *   per axis (BOX: one tap of weight S = den; BILINEAR: f = 0), so a U8 sum is den_x * den_y times the code, and a float sum
 *   lies within a binary64 rounding or two of den_x * den_y times a value that is exactly a binary32.
 *
 *   - 2D footprints only: z selects an array slice and nothing is resampled along z.  A context whose footprint is 3D
 *     (block_z > 1) returns ASTCENC_ERR_BAD_PARAM.
 *   - Entries, the window inside the image (z included), device ownership, the null / zero-count cases, the alignment of `out`,
 *     flag bits, pitches below the tight ones (of the OUTPUT size), a plane_pitch with INTERLEAVED, the format and the stream
 *     are checked as in astcenc_amd_decompress_tensors_device, with its error codes; everything is checked before anything is
 *     launched, a failure returns its error with nothing written, and the log callback names the index of the region or entry.
 *   - Also ASTCENC_ERR_BAD_PARAM: a filter that is not one of the above; a size_x, size_y, out_x or out_y that is zero or above
 *     65535; more than 2^32 - 1 work items in all.  A work item is a tile of one region's output: up to 64 output columns by
 *     up to 8 output rows -- fewer columns, down to 8, where the window is reduced so strongly that the taps of 64 columns reach
 *     more blocks than are decoded at once -- so a region has at most ceil(out_x / 8) * ceil(out_y / min(out_y, 8)) of them.  A
 *     tile decodes the blocks its taps reach; blocks at the seams of tiles are decoded by each tile that needs them. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_decompress_scaled_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	enum astcenc_amd_window_filter filter,
	const struct astcenc_amd_scaled_region* regions, unsigned int region_count,
	void* hip_stream);

/* Compressed images sampled at arbitrary coordinates straight into tensors: what a texture unit does -- "the filtered texel at
 * (x, y)" for a buffer of coordinates: the UV buffer of a rasteriser or ray caster, a warp field, a rotated or perspective
 * crop, torch.nn.functional.grid_sample -- with the image staying compressed.  A grid is out_y rows of out_x points; a grid of
 * one row is a plain list of points.
 *
 * The sampler holds for the whole call. */
enum astcenc_amd_sample_filter {
	ASTCENC_AMD_SAMPLE_NEAREST = 0,         /* the texel the point lies in */
	ASTCENC_AMD_SAMPLE_BILINEAR = 1         /* the four texels whose centres surround the point */
};
enum astcenc_amd_sample_address {
	ASTCENC_AMD_ADDRESS_CLAMP = 0,          /* a tap outside the image reads the nearest edge texel */
	ASTCENC_AMD_ADDRESS_REPEAT = 1,         /* the image tiles the plane */
	ASTCENC_AMD_ADDRESS_MIRROR = 2,         /* ... every other tile mirrored */
	ASTCENC_AMD_ADDRESS_BORDER = 3          /* a tap outside the image is +0.0 in every channel */
};
struct astcenc_amd_sampler {
	enum astcenc_amd_sample_filter filter;
	enum astcenc_amd_sample_address address_x, address_y;
};

struct astcenc_amd_sample_grid {
	unsigned int entry;                     /* index into entries[] */
	unsigned int z;                         /* the slice */
	unsigned int out_x, out_y;              /* points per row / rows of points, each 1 .. 65535 */
	const float* coords;                    /* device pointer: point (i, j) is the pair at coords[j * coord_row_pitch + 2 * i], x then y */
	size_t coord_row_pitch;                 /* in floats, even; 0 = 2 * out_x */
	void* out;                              /* device pointer: element (c = 0, j = 0, i = 0) */
	size_t row_pitch, plane_pitch;          /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Sample grids[0 .. grid_count) into tensors of `format` (astcenc_amd_decompress_tensors_device's: type, layout, channels,
 * scale, bias).  For point (i, j) of a grid, 0 <= i < out_x, 0 <= j < out_y, with the coordinates (x, y) read from `coords`,
 * and channel c < format->channels (integers are unbounded and reals are IEEE binary64 below, unless said otherwise):
 *
 *   Coordinates.  x and y are binary32 in texel units of the entry's image of W x H texels: texel k covers [k, k + 1) and its
 *     centre is k + 0.5.  Any normalisation is the caller's: torch's grid_sample with align_corners=False has g in [-1, 1] and
 *     x = (g + 1) * W / 2.  A point is VALID when both coordinates are finite and no larger than 2^30 in magnitude (2^30 itself
 *     is valid).  An invalid point has s[c] = +0.0 for every channel and then goes through "Arithmetic, storage" like any other.
 *   Taps.  Along each axis on its own, with S the image's size along it (W or H) and u the coordinate widened to binary64:
 *       NEAREST: one tap, index floor(u), weight 1.
 *       BILINEAR: t = u - 0.5 (one binary64 subtraction), i0 = floor(t), f = t - i0 (exact).  Tap 0 is index i0 with weight
 *         1.0 - f (one binary64 subtraction); tap 1 is index i0 + 1 with weight f.
 *     A tap of weight 0 (BILINEAR's tap 1 when f = 0) is not part of any sum and its texel is not read into one: a NaN or an
 *     infinity there does not reach the result -- the rule of astcenc_amd_decompress_scaled_tensors_device.
 *   Addressing of a tap index i, by the sampler's mode for that axis; the edges are the image's:
 *       CLAMP:  min(max(i, 0), S - 1).
 *       REPEAT: i mod S, the non-negative remainder.
 *       MIRROR: m = i mod 2S (non-negative); m when m < S, else 2S - 1 - m.
 *       BORDER: i when 0 <= i <= S - 1; a tap outside (on either axis) has the value +0.0 in every channel and IS part of the sum.
 *   Source.  v(kx, ky)[c] is component c of the texel astcenc_amd_decompress_regions_device writes for (kx, ky, z) of that entry:
 *     the entry's data_type and swizzle (the Z swizzle and the constants included), the context's profile, error blocks and
 *     constant-colour blocks as there; widened to binary64 (exact for U8 codes 0 .. 255, F16 and F32 values), as in the scaled
 *     call.  Entries of different data types may share a call.
 *   Sums.  r(ky) = the sum over the x taps, in tap order, of wx * v(kx, ky)[c], for every y tap; acc = the sum over the y taps,
 *     in tap order, of wy * r(ky).  A sum starts as its first product (nothing is added to a zero); every product and every sum
 *     is one IEEE binary64 operation, round to nearest even, never fused.  s[c] = (float)acc: one rounding to binary32.  There
 *     is no division: the weights of an axis sum to 1.
 *   Arithmetic, storage.  Those of astcenc_amd_decompress_tensors_device: t = s[c] * scale[c], y = t + bias[c], two binary32
 *     roundings; F32 / F16 / BF16 round to nearest even; a NaN y is stored as the type's canonical quiet NaN.
 *   Placement.  The value is element
 *       PLANAR:       c * plane_pitch + j * row_pitch + i
 *       INTERLEAVED:  j * row_pitch + i * channels + c
 *     of `out`.  A zero pitch is the tight one: row_pitch = out_x (PLANAR) or out_x * channels (INTERLEAVED); plane_pitch =
 *     row_pitch * out_y (PLANAR only).  No other element is written.
 *
 *   Consequences: NEAREST anywhere inside texel k -- k <= u < k + 1 -- reproduces texel k; BILINEAR at (kx + 0.5, ky + 0.5)
 *   reproduces texel (kx, ky) too, because f = 0 on both axes and 1.0 * v is v.  So a grid of the texel centres of a window
 *   writes, with either filter and any address mode, bit for bit what astcenc_amd_decompress_tensors_device writes for that
 *   window without flips, for U8, F16 and F32 entries.
 *
 *   Out of scope: anisotropy; gradients with respect to coordinates or texels.
 *   Mip level selection and trilinear filtering are astcenc_amd_sample_lod_tensors_device's, below; cube maps sampled by
 *   direction are astcenc_amd_sample_cube_tensors_device's; sampling along z (here z selects an array slice) and contexts of
 *   3D footprints are astcenc_amd_sample_volume_tensors_device's.
 *
 *   - Entries, z inside the image, device ownership (of `coords` too), the null / zero-count cases, the format, pitches below the
 *     tight ones, a plane_pitch with INTERLEAVED, the alignment of `out`, a null `out` and the stream are checked as in
 *     astcenc_amd_decompress_scaled_tensors_device, with its error codes; everything is checked before anything is launched, a
 *     failure returns its error with nothing written, and the log callback names the index of the grid or entry.
 *   - Also ASTCENC_ERR_BAD_PARAM: a null `sampler`; a filter or an address mode that is not one of the above; an out_x or out_y
 *     that is zero or above 65535; a `coords` not aligned to 8 bytes; an odd coord_row_pitch, or a non-zero one below 2 * out_x;
 *     a context whose footprint is 3D (block_z > 1); an entry of 2^32 - 1 blocks or more; more than 2^32 - 1 work items in all.
 *     A null `coords`: ASTCENC_ERR_BAD_CONTEXT, like a null buffer elsewhere.  Coordinates are data: none of them is an error.
 *   - A work item is a tile of tw x th points of one grid with tw * th = 64: th = min(8, out_y rounded up to a power of two) --
 *     64 x 1 for one row, 32 x 2, 16 x 4, and 8 x 8 from five rows on -- so a grid has ceil(out_x / tw) * ceil(out_y / th) of
 *     them.  A tile decodes every block its points' taps reach once, at most 256 of them, wherever they lie in the image;
 *     blocks that several tiles need are decoded by each. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_sampler* sampler,
	const struct astcenc_amd_sample_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* Compressed mip chains sampled at a level of detail per point straight into tensors: the other half of a texture unit -- "the
 * filtered texel at (u, v) at level of detail lambda" for a UV buffer and a per-pixel level of detail: a differentiable
 * rasteriser, a neural-texture trainer, a texture-space shading pass -- with every level staying compressed, the points of one
 * grid on any levels, in one launch for many grids.  A chain is level_count consecutive entries, entries[first_entry + l] being
 * level l: what astcenc_amd_compress_mip_chain_device and its kin write (one entry per level), the outputs of
 * astcenc_amd_resize_image_device compressed, or levels assembled by hand.
 *
 * The sampler holds for the whole call. */
/* (the tag astcenc_amd_mip_filter is the mip GENERATION filter's, further down: this is the filter between levels when sampling) */
enum astcenc_amd_mip_level_filter {
	ASTCENC_AMD_MIP_NEAREST = 0,            /* the one level nearest to lambda */
	ASTCENC_AMD_MIP_LINEAR = 1              /* the two levels around lambda, blended linearly: trilinear with SAMPLE_BILINEAR */
};
struct astcenc_amd_lod_sampler {
	enum astcenc_amd_sample_filter filter;  /* within a level */
	enum astcenc_amd_sample_address address_x, address_y;
	enum astcenc_amd_mip_level_filter mip_filter;
};

struct astcenc_amd_lod_grid {
	unsigned int first_entry, level_count;  /* entries[first_entry + l] is level l; 1 <= level_count <= 32 */
	unsigned int z;                         /* the slice, inside every level */
	unsigned int out_x, out_y;              /* points per row / rows of points, each 1 .. 65535 */
	const float* coords;                    /* device pointer: point (i, j) is the pair at coords[j * coord_row_pitch + 2 * i], u then v,
	                                           NORMALISED: the image is [0, 1) x [0, 1) at every level */
	size_t coord_row_pitch;                 /* in floats, even; 0 = 2 * out_x */
	const float* lod;                       /* device pointer: point (i, j) has lod[j * lod_row_pitch + i]; NULL: 0 everywhere */
	size_t lod_row_pitch;                   /* in floats; 0 = out_x */
	float lod_bias;                         /* added to every point's lod; finite */
	void* out;                              /* device pointer: element (c = 0, j = 0, i = 0) */
	size_t row_pitch, plane_pitch;          /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Sample grids[0 .. grid_count) into tensors of `format` (astcenc_amd_decompress_tensors_device's).  For point (i, j) of a grid,
 * 0 <= i < out_x, 0 <= j < out_y, with (u, v) read from `coords` and lod from `lod`, and channel c < format->channels (reals are
 * IEEE binary64 below unless said otherwise; "one operation" is one IEEE operation, round to nearest even, never fused):
 *
 *   Levels.  Level l is the image of entries[first_entry + l], W_l x H_l texels.  The levels of a chain may have any sizes --
 *     normalised coordinates make each level well defined -- and each level has its entry's data_type and swizzle; levels of
 *     different data types may share a chain.
 *   Validity.  lambda' = lod + lod_bias, one binary32 addition; lod = +0.0 when `lod` is NULL.  A point is VALID when u and v are
 *     finite and no larger than 2^14 in magnitude (2^14 itself is valid) and lambda' is not a NaN.  An invalid point has
 *     s[c] = +0.0 for every channel and then goes through "Arithmetic, storage" like any other.  No level is larger than 65536
 *     along x or y (see below), so every level coordinate stays within the 2^30 the sample call allows.
 *   Level of detail.  lambda_c = min(max(lambda', 0), level_count - 1); the infinities clamp.
 *       MIP_NEAREST: one level, l = ceil(lambda_c + 0.5) - 1 (the sum is one binary64 addition; it selects what the exact sum
 *         would) -- the GL rule, the finer level on a tie: 0.5 selects level 0 -- with weight 1.
 *       MIP_LINEAR: l0 = floor(lambda_c), g = lambda_c - l0 (exact).  Level l0 has weight 1.0 - g (one binary64 subtraction),
 *         level l0 + 1 has weight g.  When g = 0 -- which includes l0 = level_count - 1 -- level l0 + 1 is not part of the sum and
 *         none of its blocks is read: a NaN there does not reach the result (the zero-weight rule of the sample call's taps).
 *   Within a level.  x_l = (double)u * (double)W_l and y_l = (double)v * (double)H_l: exact products (24 bits by 17).  s_l[c] is
 *     exactly what astcenc_amd_sample_tensors_device defines as s[c] for that entry and slice z, with x_l and y_l in the place of
 *     "the coordinate widened to binary64": the same taps under `filter`, the same addressing, BORDER rule, source texels and
 *     order of sums, and one rounding to binary32.
 *   Blend.  One level: s[c] = s_l[c].  Two levels: s[c] = (float)((1.0 - g) * (double)s_l0[c] + g * (double)s_l1[c]): two
 *     products and one sum, one operation each, then one rounding to binary32.
 *   Arithmetic, storage, placement.  Those of astcenc_amd_sample_tensors_device.
 *
 *   Consequences: with a chain of one level, or wherever lambda' is an integer (or beyond either end of the chain), the result is
 *   that level's s_l under either mip filter.  Where W_l and H_l are powers of two, u * W_l and v * H_l are binary32 values, so
 *   the bytes are those astcenc_amd_sample_tensors_device writes for that entry at (u * W_l, v * H_l).
 *
 *   Out of scope: level selection from coordinate derivatives (a log2 cannot be given a bit-exact contract: the caller supplies
 *   lambda); anisotropy.  Gradients with respect to the coordinates and the levels of detail are
 *   astcenc_amd_sample_lod_grad_device's, below; gradients with respect to texels are out of scope (the texels are compressed).
 *   Cube maps sampled by direction, seamless across faces, are astcenc_amd_sample_cube_tensors_device's, below; sampling along
 *   z and contexts of 3D footprints are astcenc_amd_sample_volume_tensors_device's.
 *
 *   - Everything astcenc_amd_sample_tensors_device checks is checked here with the same error codes -- the entries, the format,
 *     the sampler's filter and address modes, out_x and out_y, `coords` and its pitch, `out` and its pitches, device ownership,
 *     the context's footprint, the work items -- everything before anything is launched; a failure returns its error with
 *     nothing written, and the log callback names the index: "grid i of n".
 *   - Also ASTCENC_ERR_BAD_PARAM: a null `sampler` or a mip_filter that is not one of the above; a level_count of 0 or above 32;
 *     first_entry + level_count beyond entry_count; a z outside any level of the chain; a level (an entry used as one) with
 *     dim_x or dim_y above 65536; a lod_bias that is not finite; a `lod` not aligned to 4 bytes; a non-zero lod_row_pitch below
 *     out_x; a `lod` that is not on the device of entry 0's blocks (as `coords`).  A null `lod` is legal.  Coordinates and levels
 *     of detail are data: none of them is an error.
 *   - A work item is a tile of 64 points, those of astcenc_amd_sample_tensors_device.  A tile runs one pass per distinct level
 *     its points need, at most level_count of them (counted on a 1920 x 1080 grid whose lambda rises over four levels: 2.02 a
 *     tile), and a pass decodes every block of that level its points' taps reach once. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_lod_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_lod_sampler* sampler,
	const struct astcenc_amd_lod_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* The gradients of astcenc_amd_sample_lod_tensors_device with respect to its inputs: the backward pass of a differentiable
 * rasteriser or a neural-texture trainer over mip chains that stay compressed.  The texels are compressed and fixed, so the
 * gradients that exist are those for the coordinates and the level of detail; bilinear sampling is piecewise linear in (u, v)
 * and the blend is piecewise linear in lambda, so they have an exact form.  For every point of every grid the call takes an
 * upstream gradient -- d loss / d out, in the forward call's format and layout -- and writes d loss / d (u, v) and, when wanted,
 * d loss / d lod: the vector-Jacobian product.  With level_count = 1 it is the gradient of astcenc_amd_sample_tensors_device at
 * (u W, v H). */
struct astcenc_amd_lod_grad_grid {
	unsigned int first_entry, level_count;  /* the forward grid's fields, with its meanings and limits ... */
	unsigned int z;
	unsigned int out_x, out_y;
	const float* coords;
	size_t coord_row_pitch;
	const float* lod;
	size_t lod_row_pitch;
	float lod_bias;
	const void* grad_out;                   /* device pointer: the upstream gradient, element (c = 0, j = 0, i = 0): a tensor of the format's
	                                           type and layout, placed as the forward call places `out` */
	size_t row_pitch, plane_pitch;          /* ... of grad_out, in ELEMENTS of the format's type; 0 = tightly packed */
	float* grad_coords;                     /* device pointer: point (i, j) is the pair at grad_coords[j * grad_coord_row_pitch + 2 * i],
	                                           d loss / du then d loss / dv */
	size_t grad_coord_row_pitch;            /* in floats, even; 0 = 2 * out_x */
	float* grad_lod;                        /* device pointer: point (i, j) has grad_lod[j * grad_lod_row_pitch + i]; NULL: not wanted */
	size_t grad_lod_row_pitch;              /* in floats; 0 = out_x */
};

/* The gradients of grids[0 .. grid_count).  `format` and `sampler` are the forward call's; format->scale is used and
 * format->bias is not (a shift has no derivative).  For point (i, j) of a grid, with (u, v), lod and lod_bias as in the forward
 * call (reals are IEEE binary64 below unless said otherwise; "one operation" is one IEEE operation, round to nearest even, never
 * fused; any sum starts as its first product -- nothing is added to a zero):
 *
 *   Validity, lambda', lambda_c, l0, g.  Those of astcenc_amd_sample_lod_tensors_device.  An invalid point writes +0.0 to all
 *     three gradients.
 *   Upstream.  a[c] = (double)grad_out[c] * (double)scale[c], one product, for c < format->channels; the element of grad_out is
 *     where the forward call places out[c] of the point, and is widened exactly (F32, F16, BF16).  Upstream values are data: a NaN
 *     or an infinity there is not an error.
 *   Per level l that is part of the point (below), with x = (double)u * (double)W_l and y = (double)v * (double)H_l (exact):
 *     s_l[c] is the forward call's level sample, binary32.  S_l = the sum over c < channels, in order, of a[c] * (double)s_l[c].
 *     Under NEAREST, Dx_l = Dy_l = +0.0.
 *     Under BILINEAR, ix0 = floor(x - 0.5) and iy0 = floor(y - 0.5), wx and wy the forward call's weights.  The difference along
 *     x always uses both indices ix0 and ix0 + 1, each through the forward call's "Addressing" -- kx0 and kx1; a BORDER tap
 *     outside is +0.0 -- even where the forward call's tap 1 has weight 0; along y likewise with ky0 and ky1.
 *       d(ky) = v(kx1, ky)[c] - v(kx0, ky)[c] (one subtraction of the widened texels) for every forward y tap, in tap order, taps
 *         of weight zero left out as in the forward call: dsdx[c] = wy0 * d(ky0) [+ wy1 * d(ky1)].
 *       e(kx) = v(kx, ky1)[c] - v(kx, ky0)[c] over the forward x taps: dsdy[c] = wx0 * e(kx0) [+ wx1 * e(kx1)].
 *       Dx_l = (the sum over c < channels, in order, of a[c] * dsdx[c]) * (double)W_l, and Dy_l likewise with dsdy and H_l.
 *     A texel that is in none of these sums may or may not be read; a NaN there does not reach a result.
 *   grad_coords.  One level (g = 0, or MIP_NEAREST): (float)Dx_l0 and (float)Dy_l0.  Two levels (g != 0):
 *     (float)((1.0 - g) * Dx_l0 + g * Dx_l1) -- two products, one sum, one rounding to binary32 -- and likewise for v.
 *   grad_lod.  The derivative is not zero only under MIP_LINEAR where 0 <= lambda' < level_count - 1, that is where lambda' is not
 *     clamped: there it is (float)(S_(l0+1) - S_l0), one subtraction and one rounding -- at an integer lambda' the right
 *     derivative.  This case samples level l0 + 1 for S alone even when g = 0.  Everywhere else -- MIP_NEAREST, a clamped lambda',
 *     a chain of one level -- grad_lod is +0.0.  When grad_lod is NULL a level of weight zero is not read.
 *   Storage.  A gradient that is a NaN is stored as the canonical quiet NaN 0x7FC00000.
 *   Placement and pitches.  grad_coords as `coords`, grad_lod as `lod`.  No other element is written.
 *
 *   Consequences: under CLAMP a point more than half a texel outside the image has a zero gradient along that axis, because
 *   both taps clamp to one texel.  The same formula is the derivative under REPEAT, MIRROR and BORDER, because addressing acts
 *   on tap indices.  At a texel centre (f = 0) the gradient is the right-hand difference.  Away from cell boundaries and integer
 *   lambda the gradients agree with central differences of the forward call to within its own rounding.
 *
 *   Out of scope: gradients with respect to texels; second derivatives; the cube sampler.  The volume sampler's gradients are
 *   astcenc_amd_sample_volume_grad_device's, further down.
 *
 *   - Everything astcenc_amd_sample_lod_tensors_device checks is checked here with its error codes, grad_out in the place of
 *     `out`; the log callback names the index: "grid i of n".
 *   - ASTCENC_ERR_BAD_CONTEXT: a null grad_out or grad_coords.  ASTCENC_ERR_BAD_PARAM: a grad_coords not aligned to 8 bytes; a
 *     grad_out not aligned to its element; a grad_lod not aligned to 4 bytes; a gradient pitch below the tight one, or an odd
 *     grad_coord_row_pitch; a grad_out, grad_coords or grad_lod that is not on the device of entry 0's blocks.  A null grad_lod is
 *     legal.
 *   - Everything is checked before anything is launched; a failure writes nothing.  An output that overlaps an input is the
 *     caller's error and is not detected.
 *   - A work item is the forward call's tile of 64 points; a tile runs one pass per distinct level its points need. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_lod_grad_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_lod_sampler* sampler,
	const struct astcenc_amd_lod_grad_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* Compressed cube maps sampled by direction at a level of detail per point straight into tensors: the environment lookup of a
 * texture unit -- "the filtered texel in direction d at level of detail lambda" for a buffer of directions: the reflection
 * vectors of a probe lookup, the view rays of a sky box, the normals of an environment-lighting pass of a neural-texture
 * trainer -- with every level staying compressed and no seam along the cube's edges: a bilinear tap that leaves a face reads
 * the neighbouring face, by the "Cube edges" rule the mip filters generate the chain with (ASTCENC_AMD_MIP_EDGE_CUBE, further
 * down).  A chain is level_count consecutive entries as in astcenc_amd_sample_lod_tensors_device; a chain of one level with a
 * NULL `lod` is a cube without mips.
 *
 * The sampler holds for the whole call.  A cube has no address modes: its edges are its neighbours'. */
struct astcenc_amd_cube_sampler {
	enum astcenc_amd_sample_filter filter;          /* NEAREST or BILINEAR within a level */
	enum astcenc_amd_mip_level_filter mip_filter;   /* MIP_NEAREST or MIP_LINEAR between levels */
};

struct astcenc_amd_cube_grid {
	unsigned int first_entry, level_count;  /* entries[first_entry + l] is level l; 1 <= level_count <= 32 */
	unsigned int cube;                      /* layers 6 * cube .. 6 * cube + 5 of every level: +X, -X, +Y, -Y, +Z, -Z */
	unsigned int out_x, out_y;              /* points per row / rows of points, each 1 .. 65535 */
	const float* dirs;                      /* device pointer: point (i, j) is the triple at dirs[j * dir_row_pitch + 3 * i], dx, dy, dz;
	                                           any length but zero */
	size_t dir_row_pitch;                   /* in floats; 0 = 3 * out_x */
	const float* lod;                       /* device pointer: point (i, j) has lod[j * lod_row_pitch + i]; NULL: 0 everywhere */
	size_t lod_row_pitch;                   /* in floats; 0 = out_x */
	float lod_bias;                         /* added to every point's lod; finite */
	void* out;                              /* device pointer: element (c = 0, j = 0, i = 0) */
	size_t row_pitch, plane_pitch;          /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Sample grids[0 .. grid_count) into tensors of `format` (astcenc_amd_decompress_tensors_device's).  For point (i, j) of a grid,
 * 0 <= i < out_x, 0 <= j < out_y, with d = (dx, dy, dz) read from `dirs` and lod from `lod`, and channel c < format->channels
 * (reals are IEEE binary64 below unless said otherwise; "one operation" is one IEEE operation, round to nearest even, never
 * fused; the division is a true division):
 *
 *   Levels.  Level l is the image of entries[first_entry + l]: dim_x == dim_y == s_l <= 65536, dim_z % 6 == 0 and
 *     6 * cube + 5 < dim_z.  Layer 6 * cube + f is face f, in the face order and with the face frames (M_f, S_f, T_f) of the
 *     "Cube edges" table below.  The levels of a chain may have any sizes and data types.
 *   Validity.  lambda' = lod + lod_bias, one binary32 addition; lod = +0.0 when `lod` is NULL.  A point is VALID when dx, dy and
 *     dz are finite, not all three are zero (zeros of either sign), and lambda' is not a NaN.  There is no magnitude limit:
 *     subnormals widen exactly, and the quotient below is at most 1 in magnitude.  An invalid point has s[c] = +0.0 for every
 *     channel and then goes through "Arithmetic, storage" like any other.
 *   Face.  With a = |dx|, b = |dy|, c = |dz|: the major axis is x when a >= b and a >= c; otherwise y when b >= c; otherwise z.
 *     The face is f = 2 * axis + (1 when the major component is negative, else 0).  ma = |major component|, widened to binary64.
 *     sc = d . S_f and tc = d . T_f, each one component with a sign, so exact:
 *         f  face  sc   tc          f  face  sc   tc          f  face  sc   tc
 *         0  +X    -dz  -dy         2  +Y    +dx  +dz         4  +Z    +dx  -dy
 *         1  -X    +dz  -dy         3  -Y    +dx  -dz         5  -Z    -dx  -dy
 *   Face coordinates.  p = sc / ma and q = tc / ma, one division each (they do not depend on the level).  Per level, with
 *     h = s_l * 0.5 (exact): x = p * h + h and y = q * h + h, each one product and then one sum.  So x and y lie in [0, s_l].
 *   Taps.  NEAREST: one tap of weight 1, texel (min(floor(x), s - 1), min(floor(y), s - 1)) of face f.
 *     BILINEAR: the sample call's axis rule on x and on y: t = x - 0.5, i0 = floor(t), fr = t - i0, tap 0 is index i0 with
 *     weight 1.0 - fr, tap 1 is index i0 + 1 with weight fr.  The tap indices lie in [-1, s].  Each tap (ix, iy) reads the texel
 *     the "Cube edges" rule names for face f of a cube of s x s faces:
 *       - both indices inside [0, s): texel (ix, iy) of face f;
 *       - one index outside (it is -1 or s): the neighbouring face's texel at depth 0 from the shared edge, at the same place
 *         along the edge (the rule's overshoot k = 0);
 *       - both outside (the corner, where no face lies): the face's own corner texel (clamp(ix), clamp(iy)).  The three texels
 *         that meet at a cube corner are not averaged, as in the mip filter.
 *     A tap of weight 0 (tap 1 when fr = 0) is not part of any sum, and its block is not read.
 *   Source, sums.  Those of astcenc_amd_sample_tensors_device, the texel being (x', y', layer 6 * cube + f') of the level's entry.
 *   Level of detail, blend.  Those of astcenc_amd_sample_lod_tensors_device: lambda_c, the one level of MIP_NEAREST, the two
 *     levels and g of MIP_LINEAR, the level of weight zero that is not read, one rounding to binary32 per level and one after
 *     the blend.
 *   Arithmetic, storage, placement.  Those of astcenc_amd_sample_tensors_device.
 *
 *   Consequence: for s a power of two the direction s M_f + (2x + 1 - s) S_f + (2y + 1 - s) T_f -- the centre of texel (x, y)
 *   of face f in the doubled integer units of "Cube edges" -- reproduces that texel under either filter: the division and the
 *   product are exact, so the face coordinate is (x + 0.5, y + 0.5).  Scaling a direction by a power of two changes nothing as
 *   long as no component overflows or leaves the subnormal range inexactly.
 *
 *   Out of scope: level selection from derivatives; anisotropy; solid-angle weighting; gradients.  Contexts of 3D footprints
 *   are sampled by astcenc_amd_sample_volume_tensors_device, below (volumes, not cubes).
 *
 *   - Everything astcenc_amd_sample_lod_tensors_device checks is checked here with its error codes -- the entries, the format,
 *     the filters, out_x and out_y, the chain, lod, lod_bias and their pitch, `out` and its pitches, device ownership (of `dirs`
 *     too), the context's footprint, the work items -- everything before anything is launched; a failure returns its error with
 *     nothing written, and the log callback names the index: "grid i of n".
 *   - Also ASTCENC_ERR_BAD_PARAM: a level that is not square; a level whose dim_z % 6 != 0; a `cube` beyond a level's layers; a
 *     level with s above 65536; a `dirs` not aligned to 4 bytes; a non-zero dir_row_pitch below 3 * out_x; a `dirs` not on the
 *     device of entry 0's blocks.  A null `dirs`: ASTCENC_ERR_BAD_CONTEXT.  Directions and levels of detail are data: none of
 *     them is an error.
 *   - Work items are the lod call's tiles of 64 points and its pass per distinct level; a pass decodes every block its points'
 *     taps reach once, on whichever faces they lie. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_cube_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_cube_sampler* sampler,
	const struct astcenc_amd_cube_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* Compressed volumes sampled at (u, v, w) at a level of detail per point straight into tensors: the 3D lookup of a texture unit
 * -- "the filtered texel at (u, v, w) at level of detail lambda" for a buffer of triples: the samples of a ray marcher through a
 * CT or simulation volume, a fog or density grid, a 3D colour LUT, the feature grid of a neural field -- with every level staying
 * compressed, whether the context's footprint is 2D (the slices are compressed one by one) or one of the ten 3D footprints.  A
 * chain is level_count consecutive entries as in astcenc_amd_sample_lod_tensors_device -- what
 * astcenc_amd_compress_mip_chain_volume_device writes -- and a chain of one level with a NULL `lod` is a volume without mips.
 *
 * The sampler holds for the whole call. */
struct astcenc_amd_volume_sampler {
	enum astcenc_amd_sample_filter filter;          /* NEAREST, or BILINEAR = linear on all three axes (trilinear, 8 taps) */
	enum astcenc_amd_sample_address address_x, address_y, address_z;
	enum astcenc_amd_mip_level_filter mip_filter;   /* MIP_NEAREST or MIP_LINEAR between levels */
};

struct astcenc_amd_volume_grid {
	unsigned int first_entry, level_count;  /* entries[first_entry + l] is level l; 1 <= level_count <= 32 */
	unsigned int out_x, out_y;              /* points per row / rows of points, each 1 .. 65535 */
	const float* coords;                    /* device pointer: point (i, j) is the triple at coords[j * coord_row_pitch + 3 * i], u, v, w,
	                                           NORMALISED: the volume is [0, 1) x [0, 1) x [0, 1) at every level; 4-byte aligned */
	size_t coord_row_pitch;                 /* in floats; 0 = 3 * out_x; otherwise >= 3 * out_x */
	const float* lod;                       /* device pointer: point (i, j) has lod[j * lod_row_pitch + i]; NULL: 0 everywhere */
	size_t lod_row_pitch;                   /* in floats; 0 = out_x */
	float lod_bias;                         /* added to every point's lod; finite */
	void* out;                              /* device pointer: element (c = 0, j = 0, i = 0) */
	size_t row_pitch, plane_pitch;          /* in ELEMENTS of the format's type; 0 = tightly packed */
};

/* Sample grids[0 .. grid_count) into tensors of `format` (astcenc_amd_decompress_tensors_device's).  For point (i, j) of a grid,
 * 0 <= i < out_x, 0 <= j < out_y, with (u, v, w) read from `coords` and lod from `lod`, and channel c < format->channels (reals
 * are IEEE binary64 below unless said otherwise; "one operation" is one IEEE operation, round to nearest even, never fused):
 *
 *   Levels.  Level l is the image of entries[first_entry + l], W_l x H_l x D_l texels (dim_x, dim_y, dim_z).  The levels of a
 *     chain may have any sizes, none above 65536 along any axis, and each level has its entry's data_type and swizzle.  With a
 *     2D footprint the slices of an entry are block layers of depth 1, as everywhere in this interface; with a 3D footprint the
 *     blocks are block_z slices deep and the last layer may be partial.
 *   Validity.  lambda' = lod + lod_bias, one binary32 addition; lod = +0.0 when `lod` is NULL.  A point is VALID when u, v and w
 *     are finite and no larger than 2^14 in magnitude (2^14 itself is valid) and lambda' is not a NaN.  An invalid point has
 *     s[c] = +0.0 for every channel and then goes through "Arithmetic, storage" like any other.
 *   Level of detail.  That of astcenc_amd_sample_lod_tensors_device: lambda_c, the one level of MIP_NEAREST, the two levels and
 *     g of MIP_LINEAR, the level of weight zero that is not part of the sum and none of whose blocks is read.
 *   Within a level.  x = (double)u * (double)W_l, y = (double)v * (double)H_l and z = (double)w * (double)D_l: exact products
 *     (24 bits by 17).  On each of the three axes on its own, the "Taps" rule of astcenc_amd_sample_tensors_device with the
 *     level's size along that axis: NEAREST has one tap, index floor(x), weight 1; BILINEAR has t = x - 0.5, i0 = floor(t),
 *     f = t - i0, tap 0 of index i0 and weight 1.0 - f and tap 1 of index i0 + 1 and weight f.  So BILINEAR is linear on all
 *     three axes: up to 2 x 2 x 2 = 8 taps.  Each tap index goes through the sample call's "Addressing" with its own axis's
 *     mode (address_x, address_y, address_z) and size.  A BORDER tap outside on ANY of the three axes has the value +0.0 in
 *     every channel, IS part of the sums, and its block is not read.  A tap of weight 0 on any axis (tap 1 when f = 0) is not
 *     part of any sum and its block is not read.
 *   Source.  v(kx, ky, kz)[c] is component c of the texel astcenc_amd_decompress_regions_device writes for (kx, ky, kz) of the
 *     level's entry, widened to binary64, as in the sample call.
 *   Sums.  For every (y tap, z tap): a row r(ky, kz) = wx0 * v(kx0, ky, kz)[c] [+ wx1 * v(kx1, ky, kz)[c]].  For every z tap: a
 *     plane p(kz) = wy0 * r(ky0, kz) [+ wy1 * r(ky1, kz)].  Then acc = wz0 * p(kz0) [+ wz1 * p(kz1)].  The bracketed term is
 *     there when the axis has two taps.  A sum starts as its first product; every product and every sum is one operation.
 *     s_l[c] = (float)acc: one rounding to binary32 per level.
 *   Blend.  That of astcenc_amd_sample_lod_tensors_device: one level, s[c] = s_l[c]; two levels,
 *     s[c] = (float)((1.0 - g) * (double)s_l0[c] + g * (double)s_l1[c]), one rounding after the blend.
 *   Arithmetic, storage, placement.  Those of astcenc_amd_sample_tensors_device.
 *
 *   Consequences: where the z axis has one tap -- under NEAREST, and under BILINEAR where w * D_l - 0.5 is an integer, the
 *   remaining weight then being exactly 1.0 and 1.0 * p being p -- the level's sample is the sample call's for slice kz of that
 *   entry at (x, y); on a context of a 2D footprint, a grid all of whose points have one z tap of the same kz in every level
 *   they use writes the bytes astcenc_amd_sample_lod_tensors_device writes for z = kz.  Where W_l, H_l and D_l are powers of
 *   two, the texel centres ((kx + 0.5) / W_l, (ky + 0.5) / H_l, (kz + 0.5) / D_l) of a level selected with weight 1 reproduce,
 *   with either filter and any address modes, what astcenc_amd_decompress_tensors_device writes for those texels.
 *
 *   Out of scope: level selection from derivatives; anisotropy.  Gradients with respect to the coordinates and the level of detail are
 *   astcenc_amd_sample_volume_grad_device's, below; gradients with respect to texels are out of scope (the texels are compressed).
 *
 *   - Everything astcenc_amd_sample_lod_tensors_device checks is checked here with its error codes -- the entries, the format,
 *     the filters and address_x / address_y, out_x and out_y, the chain, lod, lod_bias and their pitch, `out` and its pitches,
 *     device ownership (of `coords` and `lod` too), the work items -- everything before anything is launched; a failure returns
 *     its error with nothing written, and the log callback names the index: "grid i of n".  There is no slice to check and no
 *     footprint is refused: all 2D and all 3D footprints are sampled.
 *   - Also ASTCENC_ERR_BAD_PARAM: an address_z that is not an address mode; a `coords` not aligned to 4 bytes; a non-zero
 *     coord_row_pitch below 3 * out_x; a level with dim_x, dim_y or dim_z above 65536; an entry of 2^32 - 1 blocks or more,
 *     counted as ceil(dim_x / block_x) * ceil(dim_y / block_y) * ceil(dim_z / block_z).  A null `coords`:
 *     ASTCENC_ERR_BAD_CONTEXT.  Coordinates and levels of detail are data: none of them is an error.
 *   - Work items are the lod call's tiles of 64 points and its pass per distinct level; a pass decodes every block its points'
 *     taps reach once, at most 512 of them, so with a 3D footprint the taps of a point that share a block cost one decode. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_volume_tensors_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_volume_sampler* sampler,
	const struct astcenc_amd_volume_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* The gradients of astcenc_amd_sample_volume_tensors_device with respect to its inputs: the backward pass of whatever optimises
 * coordinates through a volume lookup -- the parameters of the rays of a ray marcher, a deformation field, a camera pose, the
 * positions fed to the feature grid of a neural field -- over volumes that stay compressed.  The texels are compressed and fixed,
 * so the gradients that exist are those for the coordinates and the level of detail; trilinear sampling is linear in each of
 * u, v and w within a texel cell and the blend is piecewise linear in lambda, so they have an exact form in the eight texels the
 * forward call addresses.  For every point of every grid the call takes an upstream gradient -- d loss / d out, in the forward
 * call's format and layout -- and writes d loss / d (u, v, w) and, when wanted, d loss / d lod: the vector-Jacobian product. */
struct astcenc_amd_volume_grad_grid {
	unsigned int first_entry, level_count;  /* the forward grid's fields, with its meanings and limits ... */
	unsigned int out_x, out_y;
	const float* coords;
	size_t coord_row_pitch;
	const float* lod;
	size_t lod_row_pitch;
	float lod_bias;
	const void* grad_out;                   /* device pointer: the upstream gradient, element (c = 0, j = 0, i = 0): a tensor of the format's
	                                           type and layout, placed as the forward call places `out` */
	size_t row_pitch, plane_pitch;          /* ... of grad_out, in ELEMENTS of the format's type; 0 = tightly packed */
	float* grad_coords;                     /* device pointer: point (i, j) is the triple at grad_coords[j * grad_coord_row_pitch + 3 * i],
	                                           d loss / du, d loss / dv, then d loss / dw; 4-byte aligned, like `coords` */
	size_t grad_coord_row_pitch;            /* in floats; 0 = 3 * out_x; otherwise >= 3 * out_x */
	float* grad_lod;                        /* device pointer: point (i, j) has grad_lod[j * grad_lod_row_pitch + i]; NULL: not wanted */
	size_t grad_lod_row_pitch;              /* in floats; 0 = out_x */
};

/* The gradients of grids[0 .. grid_count).  `format` and `sampler` are the forward call's; format->scale is used and
 * format->bias is not (a shift has no derivative).  For point (i, j) of a grid, with (u, v, w), lod and lod_bias as in the
 * forward call (reals are IEEE binary64 below unless said otherwise; "one operation" is one IEEE operation, round to nearest
 * even, never fused; any sum starts as its first product -- nothing is added to a zero):
 *
 *   Validity, lambda', lambda_c, l0, g.  Those of astcenc_amd_sample_volume_tensors_device.  An invalid point writes +0.0 to all
 *     four gradients.
 *   Upstream.  a[c] = (double)grad_out[c] * (double)scale[c], one product, for c < format->channels; the element of grad_out is
 *     where the forward call places out[c] of the point, and is widened exactly (F32, F16, BF16).  format->bias is not used.
 *     Upstream values are data: a NaN or an infinity there is not an error.
 *   Per level l that is part of the point (below), with x = (double)u * (double)W_l, y = (double)v * (double)H_l and
 *     z = (double)w * (double)D_l, the forward call's exact products:
 *     s_l[c] is the forward call's level sample, binary32.  S_l = the sum over c < channels, in order, of a[c] * (double)s_l[c].
 *     Under NEAREST, Dx_l = Dy_l = Dz_l = +0.0.
 *     Under BILINEAR, on every axis i0 = floor(t) with t = x - 0.5 (y - 0.5, z - 0.5), and the weights and the tap counts are
 *     the forward call's.  On every axis both indices i0 and i0 + 1 are always addressed, each through the forward call's
 *     "Addressing" with that axis's mode and size -- kx0 and kx1, ky0 and ky1, kz0 and kz1 -- even where the forward call's
 *     tap 1 has weight 0.  A BORDER tap outside on any of the three axes is +0.0.  The sums mirror the forward order: the
 *     innermost runs over the first remaining axis, the outer over the next; a bracketed term is there when the forward call
 *     has two taps on that axis, and the taps are the forward call's, in tap order.
 *       dsdx[c]: d(ky, kz) = v(kx1, ky, kz)[c] - v(kx0, ky, kz)[c], one subtraction of the widened texels.  For every forward z
 *         tap: q(kz) = wy0 * d(ky0, kz) [+ wy1 * d(ky1, kz)].  dsdx[c] = wz0 * q(kz0) [+ wz1 * q(kz1)].
 *       dsdy[c]: e(kx, kz) = v(kx, ky1, kz)[c] - v(kx, ky0, kz)[c].  r(kz) = wx0 * e(kx0, kz) [+ wx1 * e(kx1, kz)].
 *         dsdy[c] = wz0 * r(kz0) [+ wz1 * r(kz1)].
 *       dsdz[c]: f(kx, ky) = v(kx, ky, kz1)[c] - v(kx, ky, kz0)[c].  r(ky) = wx0 * f(kx0, ky) [+ wx1 * f(kx1, ky)].
 *         dsdz[c] = wy0 * r(ky0) [+ wy1 * r(ky1)].
 *       Dx_l = (the sum over c < channels, in order, of a[c] * dsdx[c]) * (double)W_l; Dy_l likewise with dsdy and H_l, Dz_l with
 *         dsdz and D_l.
 *     A texel that is in none of these sums may or may not be read; a NaN there does not reach a result.
 *   grad_coords.  One level (g = 0, or MIP_NEAREST): (float)Dx_l0, (float)Dy_l0 and (float)Dz_l0.  Two levels (g != 0):
 *     (float)((1.0 - g) * Dx_l0 + g * Dx_l1) -- two products, one sum, one rounding to binary32 -- and likewise for v and w.
 *   grad_lod.  astcenc_amd_sample_lod_grad_device's rule: the derivative is not zero only under MIP_LINEAR where
 *     0 <= lambda' < level_count - 1, that is where lambda' is not clamped: there it is (float)(S_(l0+1) - S_l0), one subtraction
 *     and one rounding -- at an integer lambda' the right derivative.  This case samples level l0 + 1 for S alone even when
 *     g = 0.  Everywhere else -- MIP_NEAREST, a clamped lambda', a chain of one level -- grad_lod is +0.0.  When grad_lod is NULL
 *     a level of weight zero is not read.
 *   Storage.  A gradient that is a NaN is stored as the canonical quiet NaN 0x7FC00000.
 *   Placement and pitches.  grad_coords as `coords`, grad_lod as `lod`.  No other element is written.
 *
 *   Consequences: where the z axis has one tap, wz0 is exactly 1.0 and 1.0 * q is q; so on a context of a 2D footprint, a grid
 *   all of whose points have one z tap of the same kz in every level they use gets d loss / du, d loss / dv and grad_lod bit
 *   for bit equal to what astcenc_amd_sample_lod_grad_device writes for z = kz (and d loss / dw is the difference towards slice
 *   kz + 1 as addressed).  Under CLAMP a point more than half a texel outside the volume along an axis has a zero gradient
 *   along it, because both taps clamp to one texel.  The same formula is the derivative under REPEAT, MIRROR and BORDER,
 *   because addressing acts on tap indices.  At a texel centre on an axis the gradient along it is the right-hand difference.
 *   Away from cell boundaries and integer lambda the gradients agree with central differences of the forward call to within
 *   its own rounding.
 *
 *   Out of scope: gradients with respect to texels; second derivatives; the cube sampler.
 *
 *   - Everything astcenc_amd_sample_volume_tensors_device checks is checked here with its error codes, grad_out in the place
 *     of `out`; the log callback names the index: "grid i of n".
 *   - ASTCENC_ERR_BAD_CONTEXT: a null grad_out or grad_coords.  ASTCENC_ERR_BAD_PARAM: a grad_coords or a grad_lod not aligned to
 *     4 bytes; a grad_out not aligned to its element; a non-zero gradient pitch below the tight one (3 * out_x, out_x; the pitch
 *     of grad_coords need not be even); a grad_out, grad_coords or grad_lod that is not on the device of entry 0's blocks.  A
 *     null grad_lod is legal.
 *   - Everything is checked before anything is launched; a failure writes nothing.  An output that overlaps an input is the
 *     caller's error and is not detected.
 *   - A work item is the forward call's tile of 64 points; a tile runs one pass per distinct level its points need, and a pass
 *     decodes every block the eight addressed taps of its points reach once. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_sample_volume_grad_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_tensor_format* format,
	const struct astcenc_amd_volume_sampler* sampler,
	const struct astcenc_amd_volume_grad_grid* grids, unsigned int grid_count,
	void* hip_stream);

/* Mip chains: the levels of a 2D device image made on the device, and compressed with it in one call.
 *
 * Level i is max(1, dim_x >> i) x max(1, dim_y >> i) (the GL / Vulkan / KTX rule); level_count == 0 means the full chain down
 * to 1 x 1, floor(log2(max(dim_x, dim_y))) + 1 levels, and a level_count above that is ASTCENC_ERR_BAD_PARAM.  Level 0 is the
 * caller's image; levels 1 .. level_count - 1 are tightly packed RGBA rows of data_type in one caller buffer, each starting on a
 * 256-byte boundary.  Compressed levels lie back to back in another buffer, 16 bytes per block in raster order (ready for a KTX
 * file).
 *
 * The filter, exactly (a numpy model reproduces it bit for bit):
 *   - every level is made from the one above it; along each axis a source of S texels makes D = max(1, S >> 1), destination
 *     texel j taking: S == 1: source texel 0, weight 1, denominator 1; S even: texels 2j, 2j+1, weights (1, 1), denominator 2;
 *     S = 2n+1 > 1: texels 2j, 2j+1, 2j+2, weights (n-j, n, j+1), denominator 2n+1 (the exact area each covers).  A texel's
 *     weight is the product of its two axis weights, its denominator den = den_x * den_y;
 *   - U8, linear: sum(w * v) / den as an exact rational, rounded to nearest, ties up;
 *   - U8 in an ASTCENC_PRF_LDR_SRGB context, channels 0-2: codes decoded with the sRGB EOTF (float64, on the host), averaged in
 *     float64 as below, encoded as the number of codes c in 1..255 with mean >= EOTF((c - 0.5) / 255).  Channel 3 is linear;
 *     U8 in every other profile is linear;
 *   - F16 / F32: per y tap in increasing row, row = sum over the x taps (increasing x) of w_x * v, acc = sum over the y taps of
 *     w_y * row (each sum starting at its first product), all float64; then acc / den in float64, rounded to float32, then
 *     to F16 for F16 levels (round to nearest even both times);
 *   - channels are independent (no premultiplication: for straight-alpha textures the _weighted_ calls below weight the colour
 *     by alpha; renormalisation and coverage: the options of the _ex_ calls below);
 *     the swizzle does not touch the levels, it applies when they are compressed. */
#define ASTCENC_AMD_MAX_MIP_LEVELS 32

struct astcenc_amd_mip_chain_layout {
	unsigned int level_count;                          /* the levels of the chain (level_count resolved) */
	unsigned int dim_x[ASTCENC_AMD_MAX_MIP_LEVELS], dim_y[ASTCENC_AMD_MAX_MIP_LEVELS];
	size_t texels_offset[ASTCENC_AMD_MAX_MIP_LEVELS];  /* byte offset of level i >= 1 in device_levels; [0] = 0 (level 0 is the caller's image) */
	size_t blocks_offset[ASTCENC_AMD_MAX_MIP_LEVELS];  /* byte offset of level i's blocks in device_blocks, levels back to back */
	size_t texels_len;                                 /* bytes device_levels must hold (levels 1 .. level_count-1; 0 for one level) */
	size_t blocks_len;                                 /* bytes device_blocks must hold (all levels) */
};

/* The layout of a chain for the footprint of `config` (a 3D footprint makes one layer of blocks per 2D level).  Pure host
 * arithmetic, no device and no context: usable before any allocation.  A null config or layout, a zero dimension or an unknown
 * data_type: ASTCENC_ERR_BAD_PARAM.  So is a chain whose texel or block bytes overflow size_t. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_mip_chain_layout(
	const struct astcenc_config* config,
	unsigned int dim_x, unsigned int dim_y,
	enum astcenc_type data_type,
	unsigned int level_count,
	struct astcenc_amd_mip_chain_layout* layout);

/* Levels 1 .. level_count - 1 of the 2D device image into device_levels (levels_len bytes, at least the layout's texels_len;
 * may be null when the chain has one level).  Runs on the device that owns device_image and returns once the work on
 * hip_stream (NULL = the context's own stream) has completed.  Everything is checked before anything is launched, and an error
 * writes nothing: a null context, a bad dimension, type or level_count: ASTCENC_ERR_BAD_PARAM; a null device_image or
 * device_levels: ASTCENC_ERR_BAD_CONTEXT (as astcenc_amd_compress_image_device returns for a null buffer); levels_len too
 * short: ASTCENC_ERR_OUT_OF_MEM; a buffer or stream of another device: ASTCENC_ERR_BAD_PARAM.  The log callback
 * (astcenc_amd_set_log_callback) names the argument.  device_image needs the alignment of its components (4 bytes for U8
 * texels); device_levels must not overlap it (not checked). */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_generate_mip_chain_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y,
	enum astcenc_type data_type,
	unsigned int level_count,
	void* device_levels, size_t levels_len,
	void* hip_stream);

/* The same generation, then every level (level 0 = device_image) compressed into device_blocks (blocks_len bytes, at least the
 * layout's blocks_len) in the same chain of launches: an image set of one entry per level (astcenc_amd_compress_images_device),
 * so every level's blocks are exactly what astcenc_amd_compress_image_device writes for that level's texels, and the set's
 * rules hold -- its entry checks (before anything is launched, generation included), the alpha-scale pre-pass per level,
 * cancel, the progress callback over the whole chain's blocks.  kernel_ms covers every launch of the call, generation
 * included.  A null device_blocks: ASTCENC_ERR_BAD_CONTEXT; blocks_len too short: ASTCENC_ERR_OUT_OF_MEM; otherwise the
 * errors of generation.  The buffers must not overlap (not checked). */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_mip_chain_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	unsigned int level_count,
	void* device_levels, size_t levels_len,
	void* device_blocks, size_t blocks_len,
	void* hip_stream,
	float* kernel_ms);

/* Mip chains of texture arrays, cube maps and volumes: the 2D chain above with a third dimension.
 *
 *   - ASTCENC_AMD_MIP_ARRAY: dim_z independent 2D layers (array layers; a cube map is an array of 6 * n layers, face-major
 *     within each array element, the KTX order).  x and y halve, the layer count stays; the full chain is counted from x and y
 *     alone.  Layer l of level i is byte for byte what astcenc_amd_generate_mip_chain_device makes from layer l alone (the box
 *     filter never reads outside a face; the windowed filters below have ASTCENC_AMD_MIP_EDGE_CUBE).  A 3D footprint (block_z > 1) is ASTCENC_ERR_BAD_PARAM: its
 *     blocks would mix layers.
 *   - ASTCENC_AMD_MIP_VOLUME: one 3D image.  Level i is max(1, d >> i) on all three axes; the full chain has
 *     floor(log2(max(dim_x, dim_y, dim_z))) + 1 levels.  The filter gains a z axis with the taps of x and y: linear U8 texels
 *     weigh w_x * w_y * w_z over den_x * den_y * den_z (the exact rational mean, ties up); sRGB channels and F16 / F32 data
 *     take, per z tap in increasing slice, the 2D acc of that slice exactly as above, sum w_z * acc in float64 (starting at
 *     its first product) and divide by ((den_x * den_y) * den_z) in float64, then round as in 2D.  A volume of depth 1 makes
 *     exactly the 2D chain.
 *
 * A level is dim_z[i] slices back to back of tightly packed RGBA rows (the layout of astcenc_amd_compress_volume_device and of
 * a set entry).  Level i's blocks are exactly what astcenc_amd_compress_volume_device writes for its texels: one layer of
 * blocks per slice for a 2D footprint, ceil(dim_z[i] / block_z) layers for a 3D one.  Everything else -- level_count, the
 * 256-byte aligned texel offsets, the argument checks and their error codes, logging, stream order, cancel, progress and
 * kernel_ms -- is the 2D chain's.  A chain whose texel or block bytes overflow size_t is ASTCENC_ERR_BAD_PARAM, and so is a
 * compressed chain of more than 2^32 - 1 blocks in all (the image set's limit). */
enum astcenc_amd_mip_kind {
	ASTCENC_AMD_MIP_ARRAY = 0,
	ASTCENC_AMD_MIP_VOLUME = 1
};

struct astcenc_amd_mip_chain_volume_layout {
	unsigned int level_count;
	unsigned int dim_x[ASTCENC_AMD_MAX_MIP_LEVELS], dim_y[ASTCENC_AMD_MAX_MIP_LEVELS];
	unsigned int dim_z[ASTCENC_AMD_MAX_MIP_LEVELS];    /* layers (ARRAY) or depth (VOLUME) of level i */
	size_t texels_offset[ASTCENC_AMD_MAX_MIP_LEVELS];  /* byte offset of level i >= 1 in device_levels, 256-byte aligned; [0] = 0 */
	size_t blocks_offset[ASTCENC_AMD_MAX_MIP_LEVELS];  /* byte offset of level i's blocks in device_blocks, levels back to back */
	size_t texels_len;
	size_t blocks_len;
};

/* Host arithmetic, as astcenc_amd_mip_chain_layout; also ASTCENC_ERR_BAD_PARAM for an unknown kind, dim_z == 0, an ARRAY with
 * a 3D footprint, or a byte count beyond size_t.  A VOLUME with dim_z == 1 has the 2D layout. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_mip_chain_volume_layout(
	const struct astcenc_config* config,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	unsigned int level_count,
	struct astcenc_amd_mip_chain_volume_layout* layout);

/* Levels 1 .. level_count - 1 of device_image (dim_z slices) into device_levels: astcenc_amd_generate_mip_chain_device's
 * contract with the layout above. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_generate_mip_chain_volume_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	unsigned int level_count,
	void* device_levels, size_t levels_len,
	void* hip_stream);

/* The same generation, then every level compressed in the same chain of launches (an image set of one entry per level):
 * astcenc_amd_compress_mip_chain_device's contract with the layout above. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_mip_chain_volume_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	unsigned int level_count,
	void* device_levels, size_t levels_len,
	void* device_blocks, size_t blocks_len,
	void* hip_stream,
	float* kernel_ms);

/* Mip chain options: post-passes over the levels the calls above make.
 *
 * astcenc_amd_generate_mip_chain_ex_device and astcenc_amd_compress_mip_chain_ex_device take the arguments of their _volume_
 * counterparts plus `options` after level_count.  A null `options`, or flags == 0, gives exactly the _volume_ calls' bytes
 * (those calls, and the 2D ones, are these with null options).  Level 0, the caller's image, is never written.  The options
 * apply to levels 1 .. n-1 after the whole chain has been generated -- level i+1 is filtered from level i as the plain filter
 * made it -- so, level by level, levels(options) == post(levels(no options)).  The two options touch disjoint channels.  All
 * float arithmetic is float64, each operation rounded (no fused operations), with a true division and a correctly rounded sqrt.
 *
 *   ASTCENC_AMD_MIP_NORMALIZE (channel 3 untouched):
 *     1. decode channels 0-2: U8 v = (double)(2 code - 255) / 255.0; F16 / F32 v = 2.0 x - 1.0;
 *     2. len2 = (v0 v0 + v1 v1) + v2 v2; a texel whose len2 is 0 or not finite is written unchanged (U8 never has len2 == 0);
 *     3. n = v / sqrt(len2);
 *     4. encode: U8 code = clamp(floor((n + 1.0) * 127.5 + 0.5), 0, 255); F32 (float)((n + 1.0) * 0.5), to nearest even; F16
 *        the same float, then to half as the filter rounds.
 *   ASTCENC_AMD_MIP_ALPHA_COVERAGE (channel 3):
 *     - surfaces: one per level of a 2D image or a VOLUME, one per (level, layer) of an ARRAY (a cube face is a layer);
 *     - a texel is covered when, U8: code >= t, t = the smallest integer in 1..255 with (double)t >= (double)alpha_cutoff * 255.0;
 *       F16 / F32: (double)a >= (double)alpha_cutoff (NaN never);
 *     - a level-i surface of N texels whose level-0 surface (N0 texels) has C0 covered targets k = floor((2 C0 N + N0) / (2 N0)),
 *       computed exactly;
 *     - a_k = the k-th largest alpha of the surface (ties count individually; floats ranked by the order-preserving map of their
 *       bits, NaN below everything).  The surface is left unchanged when k == 0, or a_k <= 0 or not finite;
 *     - U8: q = floor((2 a t + a_k) / (2 a_k)) in integers; the new alpha is min(255, q) if a >= a_k, else min(t - 1, q);
 *     - F16 / F32: r = (a * alpha_cutoff) / a_k in float64, rounded to float32 (then to half for F16); a >= a_k: max(hi, min(r, 1.0)),
 *       else min(r, lo), hi / lo being the smallest / largest value of the output type that is >= / < alpha_cutoff.  A NaN
 *       alpha is written unchanged;
 *     - so a texel is covered afterwards exactly when a >= a_k: the covered count is >= k, and == k when a_k is unique.
 *
 * The options need no caller memory: the layout calls are unchanged.  The library's own scratch for them is bounded (64 MiB,
 * an array's layers being processed in groups); when it cannot be allocated the call returns ASTCENC_ERR_OUT_OF_MEM with
 * nothing written.  Errors of the options, checked with the other arguments before anything is launched, return
 * ASTCENC_ERR_BAD_PARAM with nothing written and are named "options" in the log: unknown flag bits; ALPHA_COVERAGE with an
 * alpha_cutoff that is NaN, <= 0 or > 1; NORMALIZE in an ASTCENC_PRF_LDR_SRGB context (sRGB codes are not linear vectors).
 * Everything else -- checks, stream order, cancel, progress, kernel_ms (which covers the post-passes) -- is the _volume_ calls'. */
#define ASTCENC_AMD_MIP_NORMALIZE      0x1u   /* channels 0-2 hold a unit normal (x, y, z) encoded as v = (n + 1) / 2 */
#define ASTCENC_AMD_MIP_ALPHA_COVERAGE 0x2u   /* keep channel 3's alpha-test coverage of level 0 on every level */
struct astcenc_amd_mip_options {
	unsigned int flags;      /* a set of the bits above; 0 = plain chain */
	float alpha_cutoff;      /* ALPHA_COVERAGE: the alpha test's reference value, in (0, 1] */
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_generate_mip_chain_ex_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	void* device_levels, size_t levels_len,
	void* hip_stream);

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_mip_chain_ex_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	void* device_levels, size_t levels_len,
	void* device_blocks, size_t blocks_len,
	void* hip_stream,
	float* kernel_ms);

/* Mip chain filters: windowed filters in place of the box.
 *
 * astcenc_amd_generate_mip_chain_filtered_device and astcenc_amd_compress_mip_chain_filtered_device take the arguments of the
 * _ex_ calls plus `filter` after `options`.  A null `filter`, or kind == ASTCENC_AMD_MIP_FILTER_BOX with either edge, gives exactly
 * the _ex_ calls' bytes (the box never reads outside the source, so its edge does not matter).  Level sizes, offsets and the
 * layout calls are unchanged; everything else -- the argument checks, all before anything is launched; error codes with nothing
 * written; stream order, cancel, progress and kernel_ms; the options, applied after the whole chain has been generated -- is the
 * _ex_ calls'.  An unknown kind or edge returns ASTCENC_ERR_BAD_PARAM with nothing written, named "filter" in the log.  2D images
 * are the VOLUME of depth 1; ARRAY layers are filtered independently unless the edge is CUBE ("Cube edges" below); a VOLUME's z
 * axis takes the same filter.  Every level is filtered from the level above it as stored.
 *
 * The filter, exactly (a numpy model reproduces it bit for bit):
 *   - axis geometry: a source of s texels makes d = max(1, s >> 1).  s == 1: one tap on texel 0, weight 1.0.  Otherwise
 *     r = (double)s / (double)d and destination j has the centre c = (double)((2j + 1) * s) / (double)(2d) (the product in 64-bit
 *     integers); its taps are every integer i with |t| < S, t = (((double)i + 0.5) - c) / r, in increasing i, S the support;
 *     f is evaluated on a = |t|, and w_i = f_i / sum, sum = f_first + ... in increasing i.  Tap i reads source texel
 *     clamp(i, 0, s - 1) (CLAMP) or the non-negative i mod s (WRAP); CUBE maps x and y together (below); taps on the same texel
 *     are not merged;
 *   - the functions, a2 = a * a, a3 = a2 * a, every operation a separate IEEE double operation in the order written:
 *       MITCHELL (B = C = 1/3, S = 2): a < 1: ((7.0 * a3 - 12.0 * a2) + 16.0 / 3.0) / 6.0,
 *                                      else ((((-7.0 / 3.0) * a3 + 12.0 * a2) - 20.0 * a) + 32.0 / 3.0) / 6.0;
 *       LANCZOS3 (S = 3): sinc(a) * sinc(a / 3.0);
 *       KAISER (S = 3): q = a / 3.0; (sinc(a) * I0(4.0 * sqrt(1.0 - q * q))) / I0(4.0);
 *     sinc(x) = 1.0 for x == 0, else sin(px) / px, px = 3.141592653589793 * x, sin the C library's; I0(x): q2 = (x * 0.5) *
 *     (x * 0.5), term = sum = 1.0, then for k = 1 .. 24: term = (term * q2) / (double)(k * k), sum = sum + term.  The weights are
 *     computed on the host, once per call; the device never evaluates a transcendental;
 *   - per texel, in float64: for each z tap in increasing order and each y tap in increasing order row = sum_x w_x v; per slice
 *     acc = sum_y w_y row; then vol = sum_z w_z acc.  Each sum starts at its first product; each multiply and add is rounded on
 *     its own (no fused operations); no padding taps (a zero weight would turn -0.0 into +0.0 and inf into NaN).  An ARRAY layer
 *     (and a 2D image) has the one z tap of weight 1.0;
 *   - values and results: U8 v = (double)code, result clamp(floor(vol + 0.5), 0, 255); U8 in an ASTCENC_PRF_LDR_SRGB context,
 *     channels 0-2: v = EOTF(code / 255) (the box filter's float64 table), result the number of codes c in 1..255 with
 *     vol >= EOTF((c - 0.5) / 255), channel 3 linear; F32 (float)vol; F16 that float to half (round to nearest even both times).
 *     Float data is not clamped: negative lobes may ring.
 *
 * Cube edges (ASTCENC_AMD_MIP_EDGE_CUBE): a tap that leaves a cube face reads the neighbouring face, so that both sides of a cube
 * edge are filtered from the same data.  CLAMP smears a face's border texel outwards and WRAP reads the opposite side of the same
 * face; either shows as a line along the cube's edges in sky boxes and reflection probes.
 *   - Where it is valid: kind == ASTCENC_AMD_MIP_ARRAY, dim_x == dim_y and dim_z % 6 == 0.  Anything else returns
 *     ASTCENC_ERR_BAD_PARAM with nothing written, named "filter" in the log, checked with the other arguments before anything is
 *     launched.  The check applies to every filter kind, the box included; a valid CUBE with ASTCENC_AMD_MIP_FILTER_BOX gives
 *     exactly the _ex_ calls' bytes through the box kernels, as the other edges do.
 *   - Layers: layer l is face l % 6 of cube l / 6, faces in the KTX / GL order +X, -X, +Y, -Y, +Z, -Z.  Cubes never read each
 *     other.
 *   - Face frames: face f has a major axis M_f and the directions S_f (x grows along it) and T_f (y grows along it), the GL
 *     cube-map table:
 *         f  face  M           S           T
 *         0  +X    ( 1, 0, 0)  ( 0, 0,-1)  ( 0,-1, 0)
 *         1  -X    (-1, 0, 0)  ( 0, 0, 1)  ( 0,-1, 0)
 *         2  +Y    ( 0, 1, 0)  ( 1, 0, 0)  ( 0, 0, 1)
 *         3  -Y    ( 0,-1, 0)  ( 1, 0, 0)  ( 0, 0,-1)
 *         4  +Z    ( 0, 0, 1)  ( 1, 0, 0)  ( 0,-1, 0)
 *         5  -Z    ( 0, 0,-1)  (-1, 0, 0)  ( 0,-1, 0)
 *     In doubled integer units the centre of texel (x, y) of a face of s x s texels is P = s M_f + U S_f + V T_f with
 *     U = 2x + 1 - s, V = 2y + 1 - s.
 *   - The source texel of a tap: taps, weights, tap order and every sum are those of the filter above.  Only the texel that a
 *     tap (ix, iy) of face f reads changes, for a source face of s texels:
 *       - ix and iy both inside [0, s): texel (ix, iy) of face f;
 *       - exactly one of them outside: the neighbouring face, unfolded flat across the shared edge.  Let A be the direction of
 *         the axis that is outside (S_f for x, T_f for y), sg = +1 when the index is >= s and -1 when it is < 0, k the overshoot
 *         (index - s or -1 - index), kk = min(k, s - 1), and W the in-range coordinate's doubled value times its direction
 *         (V T_f or U S_f).  Then P' = sg s A + (s - (2 kk + 1)) M_f + W.  The face read is the f' with M_f' = sg A, and the
 *         texel is x' = (P' . S_f' + s - 1) / 2, y' = (P' . T_f' + s - 1) / 2 (both divisions exact).  In words: overshoot k
 *         reads the neighbour's texel at depth k from the shared edge, at the same position along the edge; that texel is the
 *         mirror image of this face's own texel at depth k through the plane that holds the shared edge and the cube's centre.
 *         The depth stops at the neighbour's far side (kk): small faces have taps that reach further than one face (s = 3
 *         reaches 7 texels out);
 *       - both outside (the corner quadrant, where no face lies): the face's own corner texel, (clamp(ix), clamp(iy)) of face
 *         f.  The rule is symmetric in x and y and reads a texel that touches the corner;
 *       - s == 1 has one tap on texel 0 and never leaves the face.
 *     The neighbours this yields, for x < 0, x >= s, y < 0, y >= s: +X: +Z, -Z, +Y, -Y; -X: -Z, +Z, +Y, -Y; +Y: -X, +X, -Z, +Z;
 *     -Y: -X, +X, +Z, -Z; +Z: -X, +X, +Y, -Y; -Z: +X, -X, +Y, -Y.
 *   - Everything else is unchanged: values, the float64 row / acc sums in increasing tap order (a layer has the one z tap of
 *     weight 1.0), rounding, the sRGB tables, F16 conversion, level sizes, level i + 1 from level i as stored, the options as
 *     post-passes (coverage surfaces stay one per face), stream order, cancel, progress, kernel_ms, compression as an image set
 *     of one entry per level.  With ASTCENC_AMD_MIP_WEIGHT_ALPHA (below) the weighted values are read through the same mapping;
 *     channel 3 stays byte for byte the plain CUBE filter's.
 *   Not done: solid-angle weighting, averaging the three texels at a cube corner, or making opposite border texels equal; results
 *   are not bit-equal under rotations of the cube (the sums run in increasing x, then y).
 *
 * The taps live in library scratch (no caller memory), one row per destination texel of an odd axis and one per even axis below
 * 2^26 texels; when they exceed the library's 64 MiB scratch bound (odd axes of several hundred thousand texels) or cannot be
 * allocated, the call returns ASTCENC_ERR_OUT_OF_MEM with nothing written.
 *
 * Which filter: MITCHELL is the usual middle ground (little ringing, slightly soft); LANCZOS3 is the sharpest and rings most;
 * KAISER is close to LANCZOS3 with less ringing.  The basisu and toktx tools default to Kaiser or Lanczos. */
enum astcenc_amd_mip_filter_kind {
	ASTCENC_AMD_MIP_FILTER_BOX      = 0,   /* the exact box filter of the calls above */
	ASTCENC_AMD_MIP_FILTER_MITCHELL = 1,   /* Mitchell-Netravali, B = C = 1/3, support 2 */
	ASTCENC_AMD_MIP_FILTER_LANCZOS3 = 2,   /* sinc(t) sinc(t/3), support 3 */
	ASTCENC_AMD_MIP_FILTER_KAISER   = 3    /* sinc(t) I0(4 sqrt(1 - (t/3)^2)) / I0(4), support 3 */
};
enum astcenc_amd_mip_edge { ASTCENC_AMD_MIP_EDGE_CLAMP = 0, ASTCENC_AMD_MIP_EDGE_WRAP = 1, ASTCENC_AMD_MIP_EDGE_CUBE = 2 };
struct astcenc_amd_mip_filter {
	enum astcenc_amd_mip_filter_kind kind;
	enum astcenc_amd_mip_edge edge;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_generate_mip_chain_filtered_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	const struct astcenc_amd_mip_filter* filter,
	void* device_levels, size_t levels_len,
	void* hip_stream);

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_mip_chain_filtered_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	const struct astcenc_amd_mip_filter* filter,
	void* device_levels, size_t levels_len,
	void* device_blocks, size_t blocks_len,
	void* hip_stream,
	float* kernel_ms);

/* Mip chain weighting: colour filtered with alpha as its weight.
 *
 * The plain filter averages the four channels independently, so the colour stored under fully transparent texels -- which
 * nobody sees at level 0 -- is averaged into the visible edge of a cut-out shape and every level below 0 shows a fringe of it.
 * With ASTCENC_AMD_MIP_WEIGHT_ALPHA channels 0-2 of a destination texel are the mean of the source colours weighted by
 * tap weight x alpha.  Use it for textures with straight (non-premultiplied) alpha: foliage, decals, sprites, UI.  A texture
 * whose colour is already premultiplied by alpha wants the plain filter.
 *
 * astcenc_amd_generate_mip_chain_weighted_device and astcenc_amd_compress_mip_chain_weighted_device take the arguments of the
 * _filtered_ calls plus `weighting` after `filter`.  A null `weighting`, or weight == ASTCENC_AMD_MIP_WEIGHT_NONE, gives exactly
 * the _filtered_ calls' bytes through their kernels.  An unknown weight returns ASTCENC_ERR_BAD_PARAM with nothing written,
 * named "weighting" in the log; it is checked with the other arguments before anything is launched.  The weighting works with
 * every kind of chain, data type, filter and edge, in sRGB contexts, with both options (still post-passes over the finished
 * chain) and with compression.  Level sizes, offsets and the layout calls, the checks, error codes, stream order, cancel,
 * progress and kernel_ms are the _filtered_ calls'; level 0 is never written and level i+1 is filtered from level i as stored.
 *
 * The arithmetic, exactly (a numpy model reproduces it bit for bit).  A stored texel is (c0, c1, c2, a).  "The plain filter"
 * is the arithmetic above for the same filter, kind and type; "the plain sums" are its row / acc / vol sums: the same taps in
 * the same order, each sum starting at its first product, one rounded IEEE operation at a time, no fused operations.  Channel
 * 3 of every level is byte for byte the plain filter's; the weighting changes channels 0-2 only:
 *   - box, linear U8 (integers only): W = w_x * w_y * w_z per tap, SA = sum W a and SP_c = sum W a c, both exact.  SA > 0:
 *     (2 SP_c + SA) / (2 SA) floored, the exact weighted mean rounded to nearest, ties up (never above 255).  SA == 0: the
 *     plain filter's result;
 *   - box, U8 in an ASTCENC_PRF_LDR_SRGB context, channels 0-2: the value of a tap is (double)a * lin[c] (one rounded multiply,
 *     lin the EOTF table), volP_c the plain sums over those values before any division, SA the integer above.  SA > 0: the
 *     sRGB encode of volP_c / (double)SA.  SA == 0: the plain filter's result;
 *   - box, F16 / F32: the value of a tap is (double)a * (double)c (exact in float64), volP_c the plain sums over those values,
 *     volA the plain sums over (double)a (the plain filter's own alpha sum).  volA > 0.0: (float)(volP_c / volA), F16 that
 *     float rounded to half as the filter rounds.  Otherwise -- a zero, a negative or a NaN volA -- the plain filter's result.
 *     Nothing else is special-cased: infinities and negative alphas follow IEEE;
 *   - windowed filters: the same definitions with the normalised float64 tap weights.  Values: (double)(a * c) and (double)a
 *     for linear U8, (double)a * lin[c] for sRGB, (double)a * (double)c for floats; volP_c and volA are the plain separable
 *     sums over them.  volA > 0.0: m = volP_c / volA, and the result is clamp(floor(m + 0.5), 0, 255) for linear U8 (clamped in
 *     float64 before the conversion: a tiny volA from negative lobes can make m huge), the sRGB encode of m for sRGB,
 *     (float)m for floats.  Otherwise the plain filter's result.
 * Falling back to the plain result is the limit of the "alpha + epsilon" weight other resizers use: it keeps the colour that was
 * authored under fully transparent regions, which bilinear sampling at an edge still reads, instead of turning it black. */
enum astcenc_amd_mip_weight {
	ASTCENC_AMD_MIP_WEIGHT_NONE  = 0,      /* the plain filter of the calls above */
	ASTCENC_AMD_MIP_WEIGHT_ALPHA = 1       /* channels 0-2 weighted by channel 3 */
};
struct astcenc_amd_mip_weighting {
	enum astcenc_amd_mip_weight weight;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_generate_mip_chain_weighted_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	const struct astcenc_amd_mip_filter* filter,
	const struct astcenc_amd_mip_weighting* weighting,
	void* device_levels, size_t levels_len,
	void* hip_stream);

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_mip_chain_weighted_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	unsigned int level_count,
	const struct astcenc_amd_mip_options* options,
	const struct astcenc_amd_mip_filter* filter,
	const struct astcenc_amd_mip_weighting* weighting,
	void* device_levels, size_t levels_len,
	void* device_blocks, size_t blocks_len,
	void* hip_stream,
	float* kernel_ms);

/* Resizing a device image to any size with the mip filters.
 *
 * The chain calls above make exactly max(1, s >> 1) texels from s.  astcenc_amd_resize_image_device makes any number, with the
 * same filters (BOX included), edges (CLAMP and WRAP), weighting and arithmetic, so that an image whose level 0 has the wrong
 * size -- source art above a platform's cap, a scan that is no power of two, an atlas rescaled by an odd factor -- reaches the
 * size it ships at on the device and with bits that are specified.  Its output is an ordinary device image: pass it as
 * level 0 to any chain call.
 *
 * device_image is dim_x x dim_y x dim_z texels and device_out resize->dim_x x dim_y x dim_z, both tightly packed RGBA slices
 * back to back, the layout of every other device entry point.  kind ASTCENC_AMD_MIP_ARRAY: dim_z independent layers, every
 * one resized in x and y; resize->dim_z must equal dim_z (a 2D image is one layer).  ASTCENC_AMD_MIP_VOLUME: all three axes
 * are resized.  U8 data in an ASTCENC_PRF_LDR_SRGB context is filtered in linear light through the chain's EOTF and threshold
 * tables (channels 0-2).  The call needs no caller scratch; the taps are built on the host once per call and kept in the
 * context's own scratch.
 *
 * Checks, error codes, logging, stream rules and kernel_ms follow the _filtered_ calls: everything is checked before anything
 * is launched and an error writes nothing; the log names the argument (the new ones "resize"); the work is queued on
 * hip_stream (null: the context's own) and is complete on return; kernel_ms (may be null) receives the kernel's time.
 * ASTCENC_ERR_BAD_PARAM: a null context or `resize`, a zero source or destination dimension, an unknown kind, data type, filter
 * kind, edge or weight, ASTCENC_AMD_MIP_EDGE_CUBE (not done for resizing), an ARRAY whose layer count changes, texel bytes
 * beyond size_t, an integer box (U8 data, BOX) whose weight x value sums could leave 64 bits (den_x den_y den_z 65025 >= 2^63,
 * den below), a buffer or stream of another device.  ASTCENC_ERR_BAD_CONTEXT: a null buffer.  ASTCENC_ERR_OUT_OF_MEM: out_len
 * is too short, or the taps do not fit the library's 64 MiB scratch bound (a row of taps per destination texel of an axis, a
 * weight per tap; periodic ratios need one period).  There is no other cap on the ratio.
 *
 * The arithmetic, exactly (a numpy model reproduces it bit for bit).  Per axis a source of s texels makes d:
 *   - pass-through, s == 1 or d == s: destination j has one tap of weight 1.0, on texel 0 or on texel j.  An untouched axis is
 *     copied exactly and a resize to the same size returns the input's bytes;
 *   - windowed kinds otherwise: r = (double)s / (double)d; scale = r if d < s, else 1.0 (no widening when enlarging);
 *     c = (double)((2j + 1) s) / (double)(2d), the product in 64-bit integers; the taps are every integer i with |t| < S,
 *     t = (((double)i + 0.5) - c) / scale.  The function f, the normalisation by the running sum in increasing i and the CLAMP
 *     or WRAP mapping of i to a source texel are those of the chain's windowed filters above.  At d = max(1, s >> 1) these are
 *     the chain's taps, every float equal;
 *   - BOX otherwise: with g = gcd(s, d), s' = s / g and d' = d / g, destination j covers [j s', (j + 1) s') and source i
 *     covers [i d', (i + 1) d'); the taps are the sources with a non-empty overlap in increasing i, the weight is the integer
 *     overlap length and den = s'.  There are no edges.  At d = max(1, s >> 1) these are the chain's box weights.
 * Sums and results are the chain's, word for word.  Windowed: float64 row (x), acc (y) and vol (z) sums in increasing tap
 * order, each sum starting at its first product and each operation rounded on its own, then the stored results of the windowed
 * filters.  Box: the same sums with (double)w, then a division by ((den_x den_y) den_z) in float64; for linear U8 (and the
 * alpha channel of sRGB data) the exact rational mean rounded to nearest, ties up, in 64-bit integers.
 * ASTCENC_AMD_MIP_WEIGHT_ALPHA: the definitions of the weighting above with these taps, including the fallback to the plain
 * colour; channel 3 is byte for byte the plain resize's.  An ARRAY's z axis is the one tap of weight 1.0.
 *
 * Not done here: cube edges; the NORMALIZE and ALPHA_COVERAGE post-passes (a caller renormalises through a chain call, whose
 * options apply to the levels it makes); host-pointer input; per-layer sizes. */
struct astcenc_amd_resize {
	unsigned int dim_x, dim_y, dim_z;             /* destination size */
	struct astcenc_amd_mip_filter filter;         /* kind + edge; BOX allowed, EDGE_CUBE not */
	struct astcenc_amd_mip_weighting weighting;   /* NONE or ALPHA */
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_resize_image_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_amd_mip_kind kind,
	enum astcenc_type data_type,
	const struct astcenc_amd_resize* resize,
	void* device_out, size_t out_len,
	void* hip_stream,
	float* kernel_ms);

/* The destination size of a capped and / or power-of-two texture: integer arithmetic only, no device.  In this order:
 *   1. cap: if max_dim != 0 and L = max(dim_x, dim_y) > max_dim, the larger axis becomes max_dim and the other
 *      max(1, (v max_dim + L / 2) / L) (the aspect kept, rounded to nearest);
 *   2. power of two, per axis: NEXT the smallest power of two >= v; PREVIOUS the largest <= v; NEAREST is PREVIOUS when
 *      v - prev < 2 prev - v, else 2 prev (ties go up).  If the cap was given and the rounded value exceeds it: PREVIOUS.
 * ASTCENC_ERR_BAD_PARAM: a zero dimension, a null output, an unknown mode or a result above 2^31 (nothing is written). */
enum astcenc_amd_resize_pow2 {
	ASTCENC_AMD_POW2_NONE     = 0,
	ASTCENC_AMD_POW2_NEAREST  = 1,
	ASTCENC_AMD_POW2_NEXT     = 2,
	ASTCENC_AMD_POW2_PREVIOUS = 3
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_resize_dims(
	unsigned int dim_x, unsigned int dim_y,
	unsigned int max_dim,
	enum astcenc_amd_resize_pow2 pow2,
	unsigned int* out_x, unsigned int* out_y);

/* Error sums of two device-resident images of the same size, the quantities the reference CLI's quality
 * report is made of (ref: compute_error_metrics, Source/astcenccli_error_metrics.cpp:110-300):
 *   PSNR (LDR-RGBA)     = 10 log10(4 texels / (squared_error[0] + .. + [3]))
 *   PSNR (LDR-RGB)      = 10 log10(3 texels / (squared_error[0] + .. + [2]))
 *   alpha-weighted PSNR = the RGBA form over alpha_scaled_squared_error
 * U8 texels are compared as value / 255, F16 / F32 texels clamped to 0..65504, exactly as there.  The
 * HDR figures (mPSNR, log RMSE) come from astcenc_amd_compare_images_hdr_device below. */
struct astcenc_amd_error_sums {
	double squared_error[4];               /* per channel, image1 - image2 */
	double alpha_scaled_squared_error[4];  /* RGB differences scaled by image1's alpha first */
	double rgb_peak;                       /* largest R, G or B value of image1 */
	double texels;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compare_images_device(
	struct astcenc_context* context,
	const void* device_image1, enum astcenc_type type1,
	const void* device_image2, enum astcenc_type type2,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	void* hip_stream,
	struct astcenc_amd_error_sums* sums);

/* The HDR part of the same report (ref: Source/astcenccli_error_metrics.cpp:60-107 mpsnr_operator / mpsnr_sumdiff,
 * :262-268 the log2 terms, :389-403 the printed figures), over the f-stops fstop_lo..fstop_hi (the CLI's
 * -mpsnr option, default -10..10; both within -125..125):
 *   mPSNR (RGB)   = 10 log10(texels * 3 * (fstop_hi - fstop_lo + 1) * 255^2 / (mpsnr_squared_error[0] + [1] + [2]))
 *   LogRMSE (RGB) = sqrt((log2_squared_error[0] + [1] + [2]) / texels)
 *   PSNR (RGB normalised to peak) = PSNR (LDR-RGB) + 20 log10(rgb_peak)
 * log2 is the reference's own polynomial; the tone-mapping power is evaluated in double precision and rounded
 * to float where the reference calls libm's powf. */
struct astcenc_amd_hdr_error_sums {
	double log2_squared_error[4];    /* per channel, log2(image1) - log2(image2) */
	double mpsnr_squared_error[4];   /* per channel, summed over the f-stops */
	int fstop_lo, fstop_hi;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compare_images_hdr_device(
	struct astcenc_context* context,
	const void* device_image1, enum astcenc_type type1,
	const void* device_image2, enum astcenc_type type2,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	int fstop_lo, int fstop_hi,
	void* hip_stream,
	struct astcenc_amd_error_sums* sums,
	struct astcenc_amd_hdr_error_sums* hdr_sums);

/* Compressed blocks scored against their source image in one device pass: what a compression cost, without the decoded
 * image -- a buffer the size of the texture, written once and read once -- that the pair astcenc_amd_decompress_image_device +
 * astcenc_amd_compare_images_device needs.
 *
 * Let D be the image astcenc_amd_decompress_image_device writes for (device_blocks, dim_x, dim_y, dim_z, decode_type,
 * swizzle).  `sums` (and `hdr_sums`) are what astcenc_amd_compare_images_device (and _hdr_device) return for
 * (device_image, image_type) as image 1 and (D, decode_type) as image 2: the original is image 1, so the alpha scaling and
 * rgb_peak come from it.  D is never written: every texel is compared where the decoder would have stored it, as the bits it
 * would have stored -- the packed RGBA8 pixel, the half, the float -- so every per-texel term is bit for bit the one the two
 * calls form (an error block is magenta for U8 and NaN, compared as 0, for F16 / F32).  `texels` and `rgb_peak` are exact; the
 * fp64 sums are added in a fixed order of the kernel's own, without atomics: they agree with the two calls' to fp64 rounding
 * and are the same doubles on every run.
 *
 * device_block_errors (optional: NULL and 0): one record per block, raster block order (x, then y, then z; for a 2D
 * footprint and dim_z > 1 the blocks of slice z follow those of slice z - 1, as in the stream): the sum of squared_error
 * term c over the block's texels that lie inside the image.
 *
 *   - The context, blocks, data_len, dimensions, swizzle and image pointer are checked as in
 *     astcenc_amd_decompress_image_device, with its error codes; ASTCENC_ERR_BAD_PARAM also for a null context, swizzle or
 *     `sums` (`hdr_sums`), an unknown type, f-stops outside -125..125 or reversed; ASTCENC_ERR_OUT_OF_MEM for a non-null
 *     device_block_errors with block_errors_len below 32 bytes per block.  Everything is checked before anything is launched, and
 *     an error writes nothing.
 *   - Nothing but device_block_errors is written on the device; the original and the blocks are only read.
 *   - The work is queued on hip_stream (NULL: the context's own stream) and has completed on return.
 *   - The library's scratch for partial sums has a fixed size (9 MiB per device, allocated by the first such call and reused);
 *     ASTCENC_ERR_OUT_OF_MEM when it cannot be allocated. */
struct astcenc_amd_block_error {
	double squared_error[4];               /* per channel, original - decoded, over the block's texels inside the image */
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compare_blocks_device(
	struct astcenc_context* context,
	const void* device_blocks, size_t data_len,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type image_type,
	enum astcenc_type decode_type,
	const struct astcenc_swizzle* swizzle,
	struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	void* hip_stream,
	struct astcenc_amd_error_sums* sums);

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compare_blocks_hdr_device(
	struct astcenc_context* context,
	const void* device_blocks, size_t data_len,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type image_type,
	enum astcenc_type decode_type,
	const struct astcenc_swizzle* swizzle,
	struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	int fstop_lo, int fstop_hi,
	void* hip_stream,
	struct astcenc_amd_error_sums* sums,
	struct astcenc_amd_hdr_error_sums* hdr_sums);

/* The same for an image set -- the levels of a mip chain, the layers of an array, a batch of textures -- in one call:
 * entries[i].image is the original (read), entries[i].blocks the stream (read), nothing in an entry is written; the blocks are
 * decoded to the entry's data_type, which is also the original's type.  sums[i] holds the very doubles
 * astcenc_amd_compare_blocks_device returns for entry i alone (that call is a set of one entry), and device_block_errors
 * (optional) receives every entry's block records back to back in entry order, each entry's part as the single call writes
 * it.  The argument rules of astcenc_amd_decompress_images_device: every entry is checked as the single call checks its image
 * before anything is launched, and the log callback names a bad entry; the call runs on the device that owns entry 0's image,
 * a buffer of another device is ASTCENC_ERR_BAD_PARAM; entry_count == 0 succeeds and does nothing; a null `entries` with a
 * non-zero count, a null context or `sums`, or more than 2^32 - 1 blocks in all are ASTCENC_ERR_BAD_PARAM; a
 * block_errors_len below 32 bytes per block of the whole set is ASTCENC_ERR_OUT_OF_MEM.
 * HDR sums for sets are not provided: call astcenc_amd_compare_blocks_hdr_device per image. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compare_image_set_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	void* hip_stream,
	struct astcenc_amd_error_sums* sums);

/* Adaptive effort: re-encode only the blocks that miss a quality target.  Three calls, each usable on its own: a launch of
 * the compression kernel over a list of blocks, the selection of blocks by their error records, and a driver that chains
 * base compression -> scoring -> selection -> strong compression of the selected blocks -> scoring -> keep-the-better merge,
 * everything in device memory.
 * Each of the three has a form over an image set (below: astcenc_amd_select_blocks_set_device and its kin), which also takes a
 * block budget: "the worst N blocks of this asset, wherever they are".
 *   Not done: an HDR (log2 / mPSNR) criterion; host-pointer input; more than two tiers.
 *
 * astcenc_amd_compress_block_list_device: device_list[i], i < list_count, is a raster block index of the image (the order
 * of astcenc_amd_compress_volume_device, whose per-slice loading default and ASTCENC_AMD_OPT_PER_SLICE_FAST_LOAD apply).  For
 * every i with device_list[i] < blocks the 16 bytes at device_out + 16 * device_list[i] become exactly the bytes
 * astcenc_amd_compress_volume_device writes there for the same arguments; no other byte of device_out is written.
 *   - Indices >= blocks are skipped (a stale list never writes outside the buffer); duplicates rewrite the same bytes; any
 *     order; list_count == 0 succeeds, launches nothing and writes nothing.
 *   - Checks and error codes of astcenc_amd_compress_volume_device; data_len is checked against the whole image's blocks.
 *     Also: a null device_list with a non-zero count is ASTCENC_ERR_BAD_CONTEXT, as the other null buffers are; a list on
 *     another device than the image, or an image of more than 2^32 - 1 blocks, is ASTCENC_ERR_BAD_PARAM.  Everything is checked
 *     before anything is launched, and an error writes nothing.
 *   - A context with a_scale_radius != 0 runs the alpha-average pre-pass over the whole image, as the full call does.
 *   - The call launches the build the context launches (astcenc_amd_context_kernel_name); progress counts listed blocks,
 *     cancel works as in the full call. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_block_list_device(
	struct astcenc_context* context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	const unsigned int* device_list, unsigned int list_count,
	void* device_out, size_t data_len,
	void* hip_stream,
	float* kernel_ms);

/* The criterion a block's record (struct astcenc_amd_block_error, s = squared_error) is held against:
 *   e = ((w0*s0 + w1*s1) + w2*s2) + w3*s3        every operation a separately rounded fp64 operation in that order, none fused
 *   n = the block's texels inside the image      the footprint clipped on every axis; a 2D footprint over slices counts one slice
 *   selected  iff  e > max_mean_squared_error * (double)n      one rounded multiply; a NaN e is never selected
 * The units are those of the records: U8 as value / 255, floats clamped to 0..65504.  For equal RGBA weights a PSNR target of
 * p dB corresponds to max_mean_squared_error = 4 * 10^(-p/10). */
struct astcenc_amd_block_criterion {
	double channel_weight[4];              /* each finite and >= 0 */
	double max_mean_squared_error;         /* >= 0 or +inf; per texel, over the weighted channels */
};

/* device_list[0 .. count) receives the indices of the selected blocks of a dim_x * dim_y * dim_z image in the context's
 * footprint (the context is used for nothing else) in ascending order; nothing past `count` is written; *selected_count (a
 * host pointer, required) receives count.  The same list comes out on every run.  The work is queued on hip_stream (NULL: the
 * context's own) and has completed on return.
 *   - ASTCENC_ERR_BAD_PARAM: a null context, criterion or count pointer, a zero dimension, more than 2^32 - 1 blocks, a bad
 *     criterion (a NaN, negative or non-finite weight, a NaN or negative threshold), a buffer or stream of another device than
 *     the records'.  ASTCENC_ERR_BAD_CONTEXT: a null buffer.  ASTCENC_ERR_OUT_OF_MEM: block_errors_len < 32 bytes per block,
 *     list_len < 4 bytes per block, or no memory for the library's scratch (one word per 2048 blocks).  Nothing is written on
 *     an error. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_select_blocks_device(
	struct astcenc_context* context,
	const struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	const struct astcenc_amd_block_criterion* criterion,
	unsigned int* device_list, size_t list_len,
	void* hip_stream,
	unsigned int* selected_count);

/* The driver.  Let B0 and B1 be what astcenc_amd_compress_volume_device writes with base_context and strong_context, and E0
 * and E1 the per-block records astcenc_amd_compare_blocks_device returns for B0 and B1 against the image with decode_type ==
 * data_type and decode_swizzle.  Block i of device_out is B1[i] if block i is selected by E0[i] and e(E1[i]) < e(E0[i]), else
 * B0[i]; device_block_errors[i] (optional: NULL and 0) is the matching record, bit for bit what
 * astcenc_amd_compare_blocks_device returns for the final stream.  B1 is only ever computed for the selected blocks; with no
 * block selected the strong context launches nothing.
 *   - The two contexts must agree in footprint, profile and flags (else ASTCENC_ERR_BAD_PARAM); neither may be
 *     ASTCENC_FLG_DECOMPRESS_ONLY (ASTCENC_ERR_BAD_CONTEXT, as in compression).  The same context twice is legal and replaces
 *     nothing.  All other checks are those of the calls the driver is made of (`swizzle`: compression, both passes;
 *     `decode_swizzle`: scoring), plus ASTCENC_ERR_BAD_PARAM for a null argument other than the optional ones, a bad
 *     criterion or an unknown data_type.  They are made before anything is launched, and an error writes nothing.
 *   - Scratch: a copy of the stream, the records of the mixed stream, the base records unless device_block_errors is given,
 *     and the list: at most 16 + 64 + 4 bytes per block (and the selection's word per 2048 blocks).  It is kept with the strong
 *     context and reused; ASTCENC_ERR_OUT_OF_MEM, with nothing written, when it cannot be allocated.
 *   - Cancel and progress: each pass behaves as astcenc_amd_compress_volume_device does on its own context (the strong pass
 *     reports its listed blocks); after a cancelled base pass nothing is refined.
 *   - stats (optional): the block counts, and the elapsed kernel time of the base pass, of the strong pass, and of everything
 *     else on the stream (scoring, selection, copies, merge). */
struct astcenc_amd_adaptive_stats {
	unsigned int blocks, selected, replaced;
	float kernel_ms_base, kernel_ms_strong, kernel_ms_other;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_image_adaptive_device(
	struct astcenc_context* base_context,
	struct astcenc_context* strong_context,
	const void* device_image,
	unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
	enum astcenc_type data_type,
	const struct astcenc_swizzle* swizzle,
	const struct astcenc_swizzle* decode_swizzle,
	const struct astcenc_amd_block_criterion* criterion,
	void* device_out, size_t data_len,
	struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	void* hip_stream,
	struct astcenc_amd_adaptive_stats* stats);

/* Adaptive effort over an image set -- the levels of a mip chain, the layers of an array, a batch of textures -- with a block
 * budget.  A set is entries[0 .. entry_count) as in astcenc_amd_compress_images_device.
 *
 *   Global index.  Block g of the set counts the blocks of all entries back to back in entry order, raster order within an entry:
 *     the order in which astcenc_amd_compare_image_set_device writes device_block_errors.  At most 2^32 - 1 blocks in all.  A
 *     single image is the set of one entry, and then g is its raster block index.
 *   Candidate.  For block g in entry i, e and n are those of struct astcenc_amd_block_criterion, n taken from entry i's own
 *     dimensions and the context's footprint.  Block g is a candidate iff e > max_mean_squared_error * (double)n; a NaN e never is.
 *   Key.  k = e / (double)n, one rounded fp64 division.  A candidate has e > 0, so k is positive or +inf and never a NaN, and keys
 *     order as their 64 bit patterns do.  The mean, not e: the threshold is per texel, and a partial edge block, or the 1 x 1 level
 *     of a chain, must not rank below a full block merely for holding fewer texels.
 *   Budget.  max_blocks, or ASTCENC_AMD_NO_BLOCK_BUDGET.  With c candidates and c <= max_blocks every candidate is selected.
 *     Otherwise the selected blocks are the first max_blocks candidates in the order (key descending, global index ascending):
 *     among bit-equal keys the lowest indices win.  max_blocks == 0 selects nothing.  The list holds the selected global indices
 *     in ascending order, and it is the same list on every run.
 *
 * Common rules: everything is checked before anything is launched, an error writes nothing, the log callback names the bad
 * argument or entry index; the work is queued on hip_stream (NULL: the context's own) and has completed on return; a call runs
 * on the device that owns entry 0's image (the selection: the records), a buffer of another device is ASTCENC_ERR_BAD_PARAM.
 *
 * astcenc_amd_select_blocks_set_device: only dim_x/y/z of the entries are read, their pointers may be null.  device_list[0 ..
 * *selected_count) receives the list, nothing past it is written; *candidate_count (optional) receives c.  For one entry and no
 * budget it writes exactly the list of astcenc_amd_select_blocks_device.
 *   - Errors as astcenc_amd_select_blocks_device, per entry.  Also: entry_count == 0 succeeds with both counts 0; a null `entries`
 *     with a non-zero count, or more than 2^32 - 1 blocks in all, is ASTCENC_ERR_BAD_PARAM.  list_len must hold min(blocks of the
 *     set, max_blocks) words (ASTCENC_ERR_OUT_OF_MEM).
 *   - Scratch: 8 bytes per block (the keys), a word per 2048 blocks, and a fixed 8.2 KB (the state and the digit histograms);
 *     ASTCENC_ERR_OUT_OF_MEM when it cannot be allocated.
 *
 * astcenc_amd_compress_block_list_set_device: for every listed g below the set's total, the 16 bytes of that block in its
 * entry's `blocks` buffer become exactly what astcenc_amd_compress_images_device writes there; no other byte of any entry is
 * written.  Indices at or above the total are skipped; duplicates and any order are allowed; list_count == 0 launches nothing.
 * Entry checks as astcenc_amd_compress_images_device, list rules as astcenc_amd_compress_block_list_device.  The alpha-scale
 * pre-pass runs per entry over the whole entry; progress counts listed blocks, cancel works as in the list call.
 *
 * astcenc_amd_compress_images_adaptive_device: the driver over a set.  entries[i].blocks receives the result, entries[i].swizzle is
 * the compression swizzle, one decode_swizzle scores all entries.  Let B0 / B1 be what astcenc_amd_compress_images_device writes
 * with the base / strong context, E0 / E1 the records astcenc_amd_compare_image_set_device gives for them (entry swizzle =
 * decode_swizzle), and S the selection above on E0.  Block g of the output is B1 if g is in S and e(E1[g]) < e(E0[g]), else B0;
 * device_block_errors (optional) receives the matching records, bit for bit those of the set scoring call on the final streams.
 * B1 is computed for S only; with S empty the strong context launches nothing; after a cancelled base pass nothing is refined.
 *   - Context agreement rules and error codes of astcenc_amd_compress_image_adaptive_device.  With one entry and
 *     ASTCENC_AMD_NO_BLOCK_BUDGET the bytes, records and counts equal those of that call.
 *   - Scratch: at most 16 + 64 + 4 + 8 bytes per block of the set plus the selection's fixed part, kept with the strong context;
 *     ASTCENC_ERR_OUT_OF_MEM, with nothing written, when it cannot be allocated.
 * A mip chain needs no call of its own: the levels of any chain call are an image set. */
#define ASTCENC_AMD_NO_BLOCK_BUDGET 0xFFFFFFFFu

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_select_blocks_set_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	const struct astcenc_amd_block_criterion* criterion,
	unsigned int max_blocks,
	unsigned int* device_list, size_t list_len,
	void* hip_stream,
	unsigned int* candidate_count,
	unsigned int* selected_count);

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_block_list_set_device(
	struct astcenc_context* context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const unsigned int* device_list, unsigned int list_count,
	void* hip_stream,
	float* kernel_ms);

struct astcenc_amd_adaptive_set_stats {
	unsigned int blocks, candidates, selected, replaced;
	float kernel_ms_base, kernel_ms_strong, kernel_ms_other;
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_compress_images_adaptive_device(
	struct astcenc_context* base_context,
	struct astcenc_context* strong_context,
	const struct astcenc_amd_image_set_entry* entries, unsigned int entry_count,
	const struct astcenc_swizzle* decode_swizzle,
	const struct astcenc_amd_block_criterion* criterion,
	unsigned int max_blocks,
	struct astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
	void* hip_stream,
	struct astcenc_amd_adaptive_set_stats* stats);

/* "hip:gfx950" for the product library. */
ASTCENC_PUBLIC const char* astcenc_amd_backend_name(void);

/* Diagnostics.  The library reports through the reference's error codes and prints nothing.  What it knows beyond the code
 * -- which HIP call failed, why a device of ASTCENC_AMD_DEVICES was skipped -- is handed, one line per event and without a
 * trailing newline, to the callback installed here (process-wide; null, the default, switches it off; the callback may be
 * called from any thread that is inside a library call, and from the library's own threads -- a device's host thread, the
 * worker that waits for a run-time kernel build).  ASTCENC_AMD_LOG=stderr in the environment prints the same
 * lines to stderr when no callback is installed. */
ASTCENC_PUBLIC void astcenc_amd_set_log_callback(void (*callback)(const char* message));

/* Number of GPUs the context shards host images over.  By default astcenc_context_alloc() prepares the calling
 * thread's current device only (one process per GPU is the usual deployment, and a context must not touch its
 * neighbours' GPUs).  With the environment variable ASTCENC_AMD_DEVICES = "all" or a list of ordinals ("0,1,2,3")
 * it prepares those devices, and astcenc_compress_image() / astcenc_decompress_image() then deal contiguous ranges
 * of block rows of the host image to them -- each with its own tables, streams and PCIe pipeline -- and join them,
 * the way the reference deals blocks to its N worker threads (ref: Source/astcenc_entry.cpp:1009-1038, :1340-1385).
 * Buffers that already live on a device (the *_device entry points) are processed on the device that owns them,
 * whatever the list says. */
ASTCENC_PUBLIC int astcenc_amd_context_device_count(const struct astcenc_context* context);

/* Name of the build of the compression kernel the context launches (what a rocprofv3 kernel trace shows, without the
 * namespace).  The library holds generic builds -- "astc_compress_blocks_{ldr,hdr}64" for footprints of at most 64 texels,
 * "astc_compress_blocks_{ldr,hdr}" for the larger ones -- and builds compiled for one context each, whose LDS layout,
 * configuration and table root are compile-time constants: "astc_compress_blocks_ldr_6x6m" (6x6 -medium, LDR),
 * "astc_compress_blocks_ldr_8x8t" (8x8 -thorough, LDR), "astc_compress_blocks_hdr_6x6m" (6x6 -medium, HDR).  A context gets
 * such a build when its records equal the build's byte for byte (default flags and channel weights), the generic one
 * otherwise; both produce the same bytes.  ASTCENC_AMD_KERNEL=generic in the environment keeps every context on the
 * generic builds. */
ASTCENC_PUBLIC const char* astcenc_amd_context_kernel_name(const struct astcenc_context* context);

/* Every other context gets a build of its own at run time: the library carries its device source, writes the context's
 * records as constants, compiles the kernel with hipRTC for the device's architecture on a background thread and keeps the
 * code object on disk (ASTCENC_AMD_CACHE_DIR, else $XDG_CACHE_HOME/astcenc_amd, else ~/.cache/astcenc_amd) under a hash of
 * source, records, options and compiler version; the name is then "astc_compress_blocks_jit_<hash>".  Until that build is
 * there the context runs the generic one -- same bytes.  ASTCENC_AMD_JIT in the environment: "lazy" (default: a cached
 * build is used at once, a compile is started when the context has compressed 2^18 blocks), "eager" (started in
 * astcenc_context_alloc), "sync" (finished inside astcenc_context_alloc), "off".
 *
 * astcenc_amd_context_specialize() waits for the context's specialised build -- starting the compile if need be -- and
 * switches the context to it: ASTCENC_SUCCESS when the context now launches a specialised build (one of the library's own or
 * its run-time build), ASTCENC_ERR_NOT_IMPLEMENTED when it stays generic (no hipRTC library on the box, "off", a compile
 * error: astcenc_amd_set_log_callback says which).  Must not run concurrently with a compression on the same context. */
ASTCENC_PUBLIC enum astcenc_error astcenc_amd_context_specialize(struct astcenc_context* context);

/* Behaviour switches that have no counterpart in the reference API. */
enum astcenc_amd_option {
	/* Multi-slice RGBA8 input (image.dim_z > 1) with a 2D footprint, LDR profile and identity swizzle: the
	 * reference's fast block loader reads slice 0 for every slice (Source/astcenc_image.cpp:304), so it emits
	 * slice 0's blocks dim_z times.  0: do exactly that, byte for byte (the default of astcenc_compress_image, which
	 * promises the reference's bytes).  1: every slice is loaded from its own data, the output equals compressing the
	 * slices one by one (the default of astcenc_amd_compress_volume_device, which has no reference counterpart). */
	ASTCENC_AMD_OPT_PER_SLICE_FAST_LOAD = 1
};

ASTCENC_PUBLIC enum astcenc_error astcenc_amd_context_set_option(
	struct astcenc_context* context,
	enum astcenc_amd_option option,
	int value);

#endif
