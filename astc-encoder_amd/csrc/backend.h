// SPDX-License-Identifier: Apache-2.0
// Seam between the host API layer (astcenc_entry.cpp) and whatever executes the per-block
// compressor.  The product library links backend_hip.hip (HIP kernels on the current device).
// oracle/emu links backend_emu.cpp, which runs the same wave_*.h source sequentially on the CPU as
// a debugging aid -- it is never part of libastcenc_amd.so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <vector>
#include "astc_tables.h"
#include "image_set.h"
#include "mip_filter.h"
#include "mip_post.h"

namespace astcd {

struct Backend;

struct CompressJob {
	const void* const* host_slices; // dim_z pointers to tightly packed RGBA rows (one 2D slice each), host memory; may be null
	const void* device_data;   // the slices back to back, already resident in HBM; used when host_slices is null
	uint32_t dim_x, dim_y, dim_z;
	uint32_t data_type;        // astcenc_type
	uint32_t swz[4];
	uint8_t* host_out;         // 16 bytes per block, host memory; may be null
	uint8_t* device_out;       // HBM destination when host_out is null
	void*    stream;           // hipStream_t for the device-resident path (null = backend's own)
	float*   kernel_ms;        // optional: elapsed kernel time measured with HIP events
	uint32_t a_scale_radius;   // != 0: alpha-average pre-pass, fully transparent neighbourhoods encode as constant zero
	const std::atomic<int>* cancel_flag; // polled between chunks
	void (*progress)(float);   // optional; called with a monotonically increasing percentage
	uint32_t fast_load_slice0; // multi-slice RGBA8 / LDR / identity-swizzle input with a 2D footprint: 1 = every slice reads
	                           // slice 0 like the reference's fast loader (astcenc_image.cpp:304), 0 = each slice reads itself
	// A block-row shard of a 2D host image with the alpha-scale pre-pass: host_slices[0] starts halo_above texel rows
	// above the shard's first row and halo_below rows follow its last one (dim_y counts the shard's own rows only).  The
	// pre-pass runs over all of them, the blocks of the shard's own rows are compressed (backend_compress sets these).
	uint32_t halo_above, halo_below;
	// A block list (astcenc_amd_compress_block_list_device, device-resident jobs only; device_list null: every block of the image):
	// the list_count raster block indices at device_list are compressed into their own slots of device_out, nothing else of it
	// is written.
	const uint32_t* device_list;
	uint32_t list_count;
};

struct DecompressJob {
	const uint8_t* host_blocks;   // 16 bytes per block, raster block order
	size_t   block_bytes;
	void* const* host_slices;     // dim_z pointers to tightly packed RGBA rows (one 2D slice each) of data_type, host memory
	uint32_t dim_x, dim_y, dim_z;
	uint32_t data_type;           // astcenc_type
	uint32_t swz[4];
};

/* Decompression with both ends in device memory (emu: host memory). */
struct DecompressDeviceJob {
	const uint8_t* device_blocks;
	void*    device_image;        // dim_z slices back to back
	uint32_t dim_x, dim_y, dim_z;
	uint32_t data_type;
	uint32_t swz[4];
	void*    stream;
};

/* Geometry shared by the backends (host code only: this header is not part of the run-time build's source). */
inline size_t texel_bytes(uint32_t data_type) { return data_type == 0 ? 4 : data_type == 1 ? 8 : 16; }   // astcenc_type

/* The blocks of a job's image in the context's footprint. */
struct BlockGrid {
	uint32_t x, y, z;
	uint32_t dim_z;            // the image's slices (a job's dim_z of 0 counts as 1)
	size_t count() const { return (size_t)x * y * z; }
};
template <class Job> inline BlockGrid block_grid(const TableRoot& root, const Job& job)
{
	const uint32_t dim_z = job.dim_z ? job.dim_z : 1u;
	return { (job.dim_x + root.dim_x - 1) / root.dim_x, (job.dim_y + root.dim_y - 1) / root.dim_y, (dim_z + root.dim_z - 1) / root.dim_z, dim_z };
}

/* The reference's fast RGBA8 loader (ref: astcenc_entry.cpp:946): identity swizzle, LDR, U8 data and a 2D footprint.  Part of the
 * bit-exactness contract. */
inline bool uses_fast_load(const TableRoot& root, int32_t profile, const CompressJob& job)
{
	const bool identity = job.swz[0] == 0 && job.swz[1] == 1 && job.swz[2] == 2 && job.swz[3] == 3;
	return identity && profile < 2 && job.data_type == 0 && root.dim_z == 1;
}

/* The kernel's record of the image of `job` whose texels start at `data` (alpha_avg: null, set by the pre-pass). */
inline ImageDesc image_desc(const TableRoot& root, int32_t profile, const CompressJob& job, const void* data)
{
	const BlockGrid g = block_grid(root, job);
	ImageDesc img;
	img.data = data;
	img.dim_x = job.dim_x; img.dim_y = job.dim_y; img.dim_z = g.dim_z;
	img.data_type = job.data_type;
	for (int i = 0; i < 4; i++) img.swz[i] = job.swz[i];
	img.blocks_x = g.x; img.blocks_y = g.y; img.blocks_z = g.z;
	img.use_fast_load = uses_fast_load(root, profile, job) ? 1 : 0;
	img.fast_load_slice0 = job.fast_load_slice0;
	img.alpha_avg = nullptr;
	img.a_scale_radius = job.a_scale_radius;
	img.list = job.device_list;
	img.tickets = nullptr;
	return img;
}

/* An image set on one device (astcenc_amd_compress_images_device): every entry is described by the device-resident fields
 * of a CompressJob (device_data, device_out, dimensions, data_type, swz, a_scale_radius, fast_load_slice0); the blocks of all
 * entries are compressed as one block range, entry after entry. */
struct CompressSetJob {
	const CompressJob* entries;
	uint32_t count;            // >= 1; the blocks of all entries fit in 32 bits (checked by the caller)
	void*    stream;
	float*   kernel_ms;
	const std::atomic<int>* cancel_flag;
	void (*progress)(float);
	const struct MipChainJob* generate;   // non-null: generate this mip chain first, on the same stream (the entries are its levels)
	// A block list (astcenc_amd_compress_block_list_set_device; device_list null: every block of the set): the list_count global
	// block indices at device_list -- the blocks of all entries counted back to back -- are compressed into their own slots of
	// their entries' outputs, nothing else is written.
	const uint32_t* device_list;
	uint32_t list_count;
};

/* Levels 1 .. level_count - 1 of a device image (astcenc_amd_generate_mip_chain_device and its _volume_ form, mip_filter.h):
 * level i at device_levels + texels_offset[i]; runs on the device that owns device_image, every buffer must be there (else
 * rc 3).  kind 0 (ASTCENC_AMD_MIP_ARRAY): dim_z independent 2D layers; kind 1 (VOLUME): z halves too, a 2D image being the
 * volume of depth 1. */
struct MipChainJob {
	const void* device_image;
	uint32_t dim_x, dim_y, dim_z, kind, data_type, level_count;
	uint32_t srgb;             // U8 channels 0-2 are sRGB-encoded (an ASTCENC_PRF_LDR_SRGB context)
	uint8_t* device_levels;
	size_t texels_offset[MIP_MAX_LEVELS];
	void* stream;
	// the post-passes of levels 1 .. n-1 (mip_post.h, astcenc_amd_generate_mip_chain_ex_device): MIP_POST_* flags, 0 = none
	uint32_t post_flags;
	float alpha_cutoff;        // ALPHA_COVERAGE: the alpha test's reference value, and what the host derived from it:
	uint32_t cover_t;          //   U8: a code is covered when >= cover_t (mip_cover_u8_threshold)
	float cover_hi, cover_lo;  //   F16 / F32: the output type's values just at / below the cutoff (mip_cover_bounds)
	// the filter (mip_resample.h, astcenc_amd_generate_mip_chain_filtered_device): MIP_FILTER_* and MIP_EDGE_*; 0 = the box
	// filter of mip_filter.h
	uint32_t filter_kind, filter_edge;
	// the weighting (mip_weighted.h, astcenc_amd_generate_mip_chain_weighted_device): MIP_WEIGHT_*; 0 = none, the plain kernels
	uint32_t weight;
};

/* A device image resized to out_x x out_y x out_z (astcenc_amd_resize_image_device, mip_resize.h): kind, data_type, srgb and the
 * filter, edge and weight as in a MipChainJob; an ARRAY keeps its layers (out_z == dim_z). */
struct ResizeJob {
	const void* device_image;
	void* device_out;
	uint32_t dim_x, dim_y, dim_z, out_x, out_y, out_z, kind, data_type, srgb;
	uint32_t filter_kind, filter_edge, weight;
	void* stream;
	float* kernel_ms;
};

/* ... and its decompression (astcenc_amd_decompress_images_device): every entry as a DecompressDeviceJob (stream unused). */
struct DecompressSetJob {
	const DecompressDeviceJob* entries;
	uint32_t count;
	void*    stream;
};

/* Squared-error sums of two images of the same size (wave_metrics.h); sums[METRIC_SUMS] on the host. */
struct CompareJob {
	const void* device_a; uint32_t type_a;
	const void* device_b; uint32_t type_b;
	size_t texels;
	void* stream;
	double* sums;              // METRIC_SUMS_HOST doubles: [0..3] squared error, [4..7] alpha-scaled, [8] rgb peak, [10..13] log2, [14..17] mPSNR
	int hdr, fstop_lo, fstop_hi;   // hdr != 0: also the HDR sums over f-stops fstop_lo..fstop_hi
};
constexpr int METRIC_SUMS_HOST = 18;

/* Error sums of compressed blocks against their source images (wave_quality.h): an image set whose entries are compared
 * without a decoded image in memory.  Per entry a DecompressDeviceJob whose device_image is unused and whose data_type is the
 * type the blocks are decoded to, the original and the optional per-block output. */
struct QualityEntryJob {
	DecompressDeviceJob decode;
	const void* device_original; uint32_t original_type;
	double* device_block_errors;   // null, or four doubles per block of the entry (squared error r, g, b, a)
};
struct QualitySetJob {
	const QualityEntryJob* entries;
	uint32_t count;
	void* stream;
	double* sums;              // METRIC_SUMS_HOST doubles per entry, laid out as CompareJob::sums
	int hdr, fstop_lo, fstop_hi;
};

/* status / return codes: 0 ok, 1 out of memory, 2 no usable device / launch failure, 3 bad argument
 * (a stream of another device than the buffers).
 * backend_create builds one device slot per GPU the context may use: every visible device by default, or the
 * ordinals listed in the environment variable ASTCENC_AMD_DEVICES.  backend_compress deals contiguous ranges of
 * block rows of a host image to those devices and joins them (the reference's N worker threads, N = devices);
 * device-resident buffers are compressed on the device that owns them. */
Backend* backend_create(const uint8_t* blob, size_t blob_bytes, const DeviceConfig& cfg, int* status);
void backend_destroy(Backend* b);
int backend_device_count(const Backend* b);
int backend_compress(Backend* b, const CompressJob& job);
int backend_decompress(Backend* b, const DecompressJob& job);
int backend_decompress_device(Backend* b, const DecompressDeviceJob& job);
int backend_compare(Backend* b, const CompareJob& job);
/* Image sets run on the device that owns entry 0's buffers; a buffer of another device is rc 3.  (Product library only: the
 * entry points live in astcenc_set.cpp, which the sequential build of oracle/emu does not link.) */
int backend_compress_set(Backend* b, const CompressSetJob& job);
int backend_decompress_set(Backend* b, const DecompressSetJob& job);
/* astcenc_amd_decompress_regions_device: the entries as DecompressDeviceJobs (device_image and stream unused), the regions as the
 * kernel's launch records (DecodeRegionLaunch below).  Runs on the device that owns entry 0's blocks. */
struct DecodeRegionLaunch;
struct DecompressRegionsJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeRegionLaunch* regions;
	uint32_t region_count;
	void*    stream;
};
int backend_decompress_regions(Backend* b, const DecompressRegionsJob& job);
/* astcenc_amd_decompress_tensors_device: the same with the call's tensor format and the regions as DecodeTensorLaunch. */
struct DecodeTensorFormat;
struct DecodeTensorLaunch;
struct DecompressTensorsJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeTensorFormat* format;
	const DecodeTensorLaunch* regions;
	uint32_t region_count;
	void*    stream;
};
int backend_decompress_tensors(Backend* b, const DecompressTensorsJob& job);
/* astcenc_amd_decompress_scaled_tensors_device: the same with the call's filter and the regions as DecodeScaledLaunch. */
struct DecodeScaledLaunch;
struct DecompressScaledJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeTensorFormat* format;
	uint32_t filter;                      // astcenc_amd_window_filter
	const DecodeScaledLaunch* regions;
	uint32_t region_count;
	void*    stream;
};
int backend_decompress_scaled(Backend* b, const DecompressScaledJob& job);
/* astcenc_amd_sample_tensors_device: the same with the call's sampler and the grids as DecodeSampleLaunch. */
struct DecodeSampler;
struct DecodeSampleLaunch;
struct DecompressSampleJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeTensorFormat* format;
	const DecodeSampler* sampler;
	const DecodeSampleLaunch* grids;
	uint32_t grid_count;
	void*    stream;
};
int backend_decompress_sample(Backend* b, const DecompressSampleJob& job);
/* astcenc_amd_sample_lod_tensors_device, astcenc_amd_sample_cube_tensors_device and astcenc_amd_sample_volume_tensors_device: the
 * same with the call's level-of-detail sampler and the grids as DecodeLodLaunch; a grid uses the entries of all its levels. */
struct DecodeLodSampler;
struct DecodeLodLaunch;
struct DecompressLodJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeTensorFormat* format;
	const DecodeLodSampler* sampler;
	const DecodeLodLaunch* grids;
	uint32_t grid_count;
	void*    stream;
};
int backend_decompress_lod(Backend* b, const DecompressLodJob& job);
int backend_decompress_cube(Backend* b, const DecompressLodJob& job);
int backend_decompress_volume(Backend* b, const DecompressLodJob& job);
/* astcenc_amd_sample_lod_grad_device: the same with the grids as DecodeLodGradLaunch. */
struct DecodeLodGradLaunch;
struct DecompressLodGradJob {
	const DecompressDeviceJob* entries;
	uint32_t entry_count;
	const DecodeTensorFormat* format;
	const DecodeLodSampler* sampler;
	const DecodeLodGradLaunch* grids;
	uint32_t grid_count;
	void*    stream;
};
int backend_decompress_lod_grad(Backend* b, const DecompressLodGradJob& job);
/* astcenc_amd_sample_volume_grad_device: the same job, the grids' coordinates triples and the sampler with its address_z. */
int backend_decompress_volume_grad(Backend* b, const DecompressLodGradJob& job);
int backend_compare_blocks_set(Backend* b, const QualitySetJob& job);
/* Block selection and the adaptive driver (astcenc_adaptive.cpp, kernel_select.hip).  backend_select_blocks: the ascending list of
 * the blocks whose record meets the criterion, synchronous, *count on the host; runs on the device that owns the records.
 * backend_adaptive_refine: everything of astcenc_amd_compress_image_adaptive_device after the base pass, on the strong context. */
struct SelectJob {
	const double* device_block_errors;   // four doubles per block
	uint32_t dim_x, dim_y, dim_z;        // the image; the footprint is the context's
	uint32_t blocks;                     // ... and its blocks, as the entry point counted them
	double weight[4], max_mse;
	uint32_t* device_list;
	void* stream;
	uint32_t* count;
};
struct AdaptiveJob {
	CompressJob strong;                  // the strong pass as a device job of the whole image: device_out holds the base stream
	DecompressDeviceJob decode;          // how the streams are scored (device_image unused, data_type = the image's)
	double weight[4], max_mse;
	double* device_block_errors;         // null, or the caller's records
	uint32_t* selected; uint32_t* replaced;
	float* kernel_ms_strong; float* kernel_ms_other;   // both null or both set
};
int backend_select_blocks(Backend* b, const SelectJob& job);
/* ... and its scratch on the device that owns the image, allocated (1: out of memory) before the base pass writes anything; the
 * output and the records (null: the library's own) must live on that device (else 3). */
int backend_adaptive_reserve(Backend* b, const void* device_image, const void* device_out, const void* device_block_errors, size_t blocks);
int backend_adaptive_refine(Backend* b, const AdaptiveJob& job);
/* The same over an image set, with a block budget (block_budget.h).  backend_select_blocks_set: runs on the device that owns the
 * records; *candidates may be null.  backend_adaptive_set_reserve / _refine: the set forms of the two calls above; the refine job's
 * strong pass is a CompressSetJob whose entries' device_out hold the base streams. */
struct BudgetSetEntry;
struct SelectSetJob {
	const double* device_block_errors;   // four doubles per block of the set
	const BudgetSetEntry* entries;
	uint32_t count;
	uint32_t blocks;                     // of all entries, as the entry point counted them
	double weight[4], max_mse;
	uint32_t max_blocks;
	uint32_t* device_list;
	void* stream;
	uint32_t* candidates; uint32_t* selected;
};
struct AdaptiveSetJob {
	CompressSetJob strong;
	const QualityEntryJob* score;        // per entry: how its stream is scored (decode.device_blocks = the entry's output)
	double weight[4], max_mse;
	uint32_t max_blocks;
	double* device_block_errors;         // null, or the caller's records
	uint32_t* candidates; uint32_t* selected; uint32_t* replaced;
	float* kernel_ms_strong; float* kernel_ms_other;   // both null or both set
};
int backend_select_blocks_set(Backend* b, const SelectSetJob& job);
int backend_adaptive_set_reserve(Backend* b, const CompressSetJob& set, const void* device_block_errors, size_t blocks);
int backend_adaptive_set_refine(Backend* b, const AdaptiveSetJob& job);
int backend_generate_mips(Backend* b, const MipChainJob& job);
int backend_resize(Backend* b, const ResizeJob& job);
/* A line for the diagnostics callback (astcenc_amd_set_log_callback), printf-style. */
void backend_log(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* backend_name();
/* Where the library's diagnostics go (null: nowhere, the default; see include/astcenc_amd.h). */
void backend_set_log_callback(void (*callback)(const char* message));


/* One kernel launch over blocks [first, first + count) of an image.  The kernel exists in two
 * builds of the same source (kernel_ldr.hip / kernel_hdr.hip). */
struct KernelLaunch {
	const uint8_t* d_tab;            // table blob in HBM (with the context's DeviceConfig and LdsLayout appended)
	uint32_t lds_bytes;              // dynamic LDS per workgroup
	ImageDesc img;
	uint8_t* d_out;
	uint32_t first, count;
	void* stream;                    // hipStream_t
	unsigned long long* d_prof;      // stage timers (profiling builds) or null
	const ImageSetTable* d_set;      // null: blocks [first, first + count) of `img` into `d_out` (positions of img.list when that is set: each
	                                 // listed block goes to its own slot); else an image set's table (image_set.h): the blocks of all entries
	                                 // back to back, `img` and `d_out` unused
	uint32_t grid = 0;               // img.tickets null: `count` workgroups, one per block; else the workgroups that draw the `count`
	                                 // blocks from those heads (block_tickets.h)
};

/* Return 0 on success, a hipError_t value otherwise. `prepare` sets the dynamic-LDS attribute and
 * reports the per-workgroup LDS bytes and the LdsLayout record (<= 256 bytes) that the backend
 * appends to the device copy of the table blob together with the DeviceConfig.  `occupancy`: the workgroups of the
 * build that one CU of the current device holds at `lds_bytes` of dynamic LDS. */
int astc_kernel_prepare_ldr(const TableRoot& root, const DeviceConfig& cfg, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes);
int astc_kernel_prepare_hdr(const TableRoot& root, const DeviceConfig& cfg, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes);
int astc_kernel_launch_ldr(const KernelLaunch& k);
int astc_kernel_launch_hdr(const KernelLaunch& k);
int astc_kernel_occupancy_ldr(uint32_t lds_bytes, int* workgroups_per_cu);
int astc_kernel_occupancy_hdr(uint32_t lds_bytes, int* workgroups_per_cu);
// ... and the builds for footprints of at most 64 texels (kernel_ldr64.hip / kernel_hdr64.hip)
int astc_kernel_prepare_ldr64(const TableRoot& root, const DeviceConfig& cfg, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes);
int astc_kernel_prepare_hdr64(const TableRoot& root, const DeviceConfig& cfg, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes);
int astc_kernel_launch_ldr64(const KernelLaunch& k);
int astc_kernel_launch_hdr64(const KernelLaunch& k);
int astc_kernel_occupancy_ldr64(uint32_t lds_bytes, int* workgroups_per_cu);
int astc_kernel_occupancy_hdr64(uint32_t lds_bytes, int* workgroups_per_cu);
// ... and the fixed-context builds (kernel_ldr_6x6m.hip, kernel_ldr_8x8t.hip, kernel_hdr_6x6m.hip): `prepare` returns
// ASTC_PREPARE_NOT_THIS_CONTEXT when the context is not the one the build was compiled for
constexpr int ASTC_PREPARE_NOT_THIS_CONTEXT = -1;
#define ASTC_DECLARE_KERNEL_VARIANT(tag) \
	int astc_kernel_prepare_##tag(const TableRoot& root, const DeviceConfig& cfg, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes); \
	int astc_kernel_launch_##tag(const KernelLaunch& k); \
	int astc_kernel_occupancy_##tag(uint32_t lds_bytes, int* workgroups_per_cu);
ASTC_DECLARE_KERNEL_VARIANT(ldr_6x6m)
ASTC_DECLARE_KERNEL_VARIANT(ldr_8x8t)
ASTC_DECLARE_KERNEL_VARIANT(hdr_6x6m)
#undef ASTC_DECLARE_KERNEL_VARIANT
const char* backend_kernel_name(const Backend* b);   // the build of the compression kernel this context launches
/* Waits for the context's specialised build (compiling it now if that has not started) and switches every device of the
 * context to it.  0: the context launches a specialised build (one of the library's fixed-context builds or its own run-time
 * build); 1: it stays on the generic build (kernel_jit.h says when). */
int backend_specialize(Backend* b);

/* Alpha-average pre-pass launch (kernel_alpha.hip).  The padded tile of a region lives in LDS while it fits
 * (ALPHA_LDS_LIMIT) and otherwise in d_scratch: astc_alpha_scratch_bytes() says how much of it and for how many
 * workgroups the launch needs (0 / 0: the LDS kernel is used). */
constexpr size_t ALPHA_LDS_LIMIT = 160u * 1024u;
// tile edge of the pre-pass on a single slice (= ALPHA_TILE of wave_alpha.h, kernel_alpha.hip asserts it): the halo rows a
// block-row shard takes along are counted in these tiles (backend_compress)
constexpr uint32_t ALPHA_TILE_ROWS_2D = 32;
struct AlphaLaunch {
	const void* d_image;
	float* d_averages;
	uint32_t dim_x, dim_y, dim_z, data_type, swz_a, radius;
	float* d_scratch; uint32_t scratch_workgroups;
	void* stream;
};
size_t astc_alpha_scratch_bytes(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t radius, uint32_t* workgroups);
int astc_alpha_launch(const AlphaLaunch& a);

/* Decompression kernel launch (kernel_decode.hip). */
struct DecodeLaunch {
	const uint8_t* d_blocks;
	void* d_image;
	const void* d_tables;            // the footprint's decoder tables in HBM (astc_decode_tables_build)
	uint32_t dim_x, dim_y, dim_z, data_type, swz[4];
	uint32_t block_x, block_y, block_z, profile;
	void* stream;
};
int astc_decode_launch(const DecodeLaunch& d);
/* An image set's decode (one DecodeLaunch per entry, stream unused): astc_decode_set_build writes the table
 * (astc_decode_set_bytes(count) bytes, image_set.h) and returns the wavefront runs of all entries; astc_decode_set_launch covers
 * them from the table's device copy, in one launch unless they exceed the grid. */
size_t astc_decode_set_bytes(uint32_t count);
uint32_t astc_decode_set_build(void* out, const DecodeLaunch* entries, uint32_t count);
int astc_decode_set_launch(const void* d_table, uint32_t runs, void* stream);
/* Windows of compressed images (astcenc_amd_decompress_regions_device; decode_regions.h): one DecodeLaunch per entry (d_image and
 * stream unused) and one DecodeRegionLaunch per region, checked by the entry point: the window lies inside image `entry`, the
 * pitches are whole texels, at least a window row / slice.  astc_decode_region_runs: the work items of one region, for the entry
 * point's bound on their sum; astc_decode_regions_build writes the table (astc_decode_regions_bytes(count) bytes) and returns the
 * runs of all regions; astc_decode_regions_launch covers them from the table's device copy, as astc_decode_set_launch does. */
struct DecodeRegionLaunch {
	uint32_t entry;
	uint32_t x, y, z, size_x, size_y, size_z;
	void*    d_out;                   // the window's texel (0, 0, 0)
	size_t   row_pitch, slice_pitch;  // bytes, not 0
};
unsigned long long astc_decode_region_runs(const DecodeRegionLaunch& r, uint32_t block_x, uint32_t block_y, uint32_t block_z);
size_t astc_decode_regions_bytes(uint32_t count);
uint32_t astc_decode_regions_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeRegionLaunch* regions, uint32_t count);
int astc_decode_regions_launch(const void* d_table, uint32_t runs, void* stream);
/* Windows decoded into tensors (astcenc_amd_decompress_tensors_device; decode_tensors.h): the call's format and one
 * DecodeTensorLaunch per region, checked by the entry point -- pitches in elements of the format's type, resolved (not 0; plane
 * unused with the interleaved layout), at least the tight ones.  The work items of a region are astc_decode_region_runs of its
 * window; the table and the launch as above, the kernel build picked by the format's type and layout. */
struct DecodeTensorFormat {
	uint32_t type, layout, channels;      // astcenc_amd_tensor_type / _layout, 1..4
	float    scale[4], bias[4];
};
struct DecodeTensorLaunch {
	uint32_t entry;
	uint32_t x, y, z, size_x, size_y, size_z;
	uint32_t flags;                       // ASTCENC_AMD_TENSOR_FLIP_*
	void*    d_out;                       // element (c = 0, k = 0, j = 0, i = 0)
	size_t   row_pitch, slice_pitch, plane_pitch;
};
size_t astc_decode_tensors_bytes(uint32_t count);
uint32_t astc_decode_tensors_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format,
                                   const DecodeTensorLaunch* regions, uint32_t count);
int astc_decode_tensors_launch(const void* d_table, uint32_t runs, uint32_t type, uint32_t layout, void* stream);
/* Scaled windows decoded into tensors (astcenc_amd_decompress_scaled_tensors_device; decode_scaled.h, kernel_decode_scaled.hip):
 * the call's format and filter and one DecodeScaledLaunch per region, checked by the entry point -- 2D footprints, sizes
 * 1 .. 65535, pitches in elements, resolved, at least the tight ones of the output.  A work item is a tile of a region's output
 * (astc_decode_scaled_tiles of them: their width depends on the ratio, the entry's data type and the footprint); the table and the
 * launch as above. */
struct DecodeScaledLaunch {
	uint32_t entry;
	uint32_t x, y, z, size_x, size_y;     // the window; z: the slice
	uint32_t out_x, out_y;                // what it becomes
	uint32_t flags;                       // ASTCENC_AMD_TENSOR_FLIP_*
	void*    d_out;                       // element (c = 0, j = 0, i = 0)
	size_t   row_pitch, plane_pitch;
};
unsigned long long astc_decode_scaled_tiles(const DecodeScaledLaunch& r, uint32_t data_type, uint32_t block_x, uint32_t block_y);
size_t astc_decode_scaled_bytes(uint32_t count);
uint32_t astc_decode_scaled_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, uint32_t filter,
                                  const DecodeScaledLaunch* regions, uint32_t count);
int astc_decode_scaled_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* Images sampled at coordinates into tensors (astcenc_amd_sample_tensors_device; decode_sample.h, kernel_decode_sample.hip): the
 * call's format and sampler and one DecodeSampleLaunch per grid, checked by the entry point -- 2D footprints, sizes 1 .. 65535,
 * pitches resolved (not 0), at least the tight ones, the coordinates aligned to a pair.  A work item is a tile of 64 points of a
 * grid (astc_decode_sample_tiles of them); the table and the launch as above. */
struct DecodeSampler {
	uint32_t filter, address_x, address_y;    // astcenc_amd_sample_filter / _address
};
struct DecodeSampleLaunch {
	uint32_t entry;
	uint32_t z;                           // the slice
	uint32_t out_x, out_y;                // points per row, rows of points
	const float* d_coords;                // point (i, j): d_coords[j * coord_row_pitch + 2 i], x then y
	size_t   coord_row_pitch;             // floats
	void*    d_out;                       // element (c = 0, j = 0, i = 0)
	size_t   row_pitch, plane_pitch;
};
unsigned long long astc_decode_sample_tiles(uint32_t out_x, uint32_t out_y);
size_t astc_decode_sample_bytes(uint32_t count);
uint32_t astc_decode_sample_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeSampler& sampler,
                                  const DecodeSampleLaunch* grids, uint32_t count);
int astc_decode_sample_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* Mip chains sampled at a level of detail per point: the lod call (astcenc_amd_sample_lod_tensors_device; decode_lod.h,
 * kernel_decode_lod.hip), the cube call and the volume call below share the sampler and the launch record -- the call's format
 * and sampler and one DecodeLodLaunch per grid, checked by the entry point -- as above, and: 1 .. 32 levels, all of them entries of
 * the call no larger than 65536 along x and y that hold slice `z`, lod (when given) aligned to a float, lod_bias finite.  A
 * work item is a tile of 64 points of a grid (astc_decode_sample_tiles of them); the table -- a record per grid, then a record per
 * level of every grid, written by decode_lod.h's decode_lod_table_build for all of them -- and the launch as above. */
struct DecodeLodSampler {
	uint32_t filter, address_x, address_y;    // astcenc_amd_sample_filter / _address
	uint32_t mip_filter;                      // astcenc_amd_mip_level_filter
	uint32_t address_z;                       // the volume call's; CLAMP (0) where the call has none, as are x and y for cubes
};
struct DecodeLodLaunch {
	uint32_t first_entry, level_count;    // level l is entry first_entry + l
	uint32_t z;                           // the call's layer selector, in every level -- lod: the slice; cube: the cube, layers 6 z .. 6 z + 5; volume: 0, unused
	uint32_t out_x, out_y;                // points per row, rows of points
	const float* d_coords;                // point (i, j): lod: the pair at d_coords[j * coord_row_pitch + 2 i], u then v; cube: the triple at
	                                      // [j * coord_row_pitch + 3 i], dx, dy, dz; volume: the triple there, u, v, w
	size_t   coord_row_pitch;             // floats
	const float* d_lod;                   // point (i, j): d_lod[j * lod_row_pitch + i]; null: 0 everywhere
	size_t   lod_row_pitch;               // floats
	float    lod_bias;
	void*    d_out;                       // element (c = 0, j = 0, i = 0)
	size_t   row_pitch, plane_pitch;
};
size_t astc_decode_lod_bytes(const DecodeLodLaunch* grids, uint32_t count);
uint32_t astc_decode_lod_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                               const DecodeLodLaunch* grids, uint32_t count);
int astc_decode_lod_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* The gradients of that call (astcenc_amd_sample_lod_grad_device; decode_lod_grad.h, kernel_decode_lod_grad.hip): the forward
 * call's launch with grad_out and its pitches in the place of the output -- it is read -- and the two buffers that are written,
 * checked by the entry point: grad_coords aligned to a pair, its pitch even, grad_lod (when given) aligned to a float, the
 * pitches resolved and at least the tight ones.  Work items, table and launch as the lod call's. */
struct DecodeLodGradLaunch {
	DecodeLodLaunch lod;                  // d_out, row_pitch, plane_pitch: grad_out's
	float*   d_grad_coords;               // point (i, j): the pair at d_grad_coords[j * grad_coord_row_pitch + 2 i]; volume: the triple at [... + 3 i]
	size_t   grad_coord_row_pitch;        // floats
	float*   d_grad_lod;                  // point (i, j): d_grad_lod[j * grad_lod_row_pitch + i]; null: not wanted
	size_t   grad_lod_row_pitch;          // floats
};
/* (the forward launch of either, for what serves both: the table writer and the backend's path) */
inline const DecodeLodLaunch& decode_lod_launch_of(const DecodeLodLaunch& g) { return g; }
inline const DecodeLodLaunch& decode_lod_launch_of(const DecodeLodGradLaunch& g) { return g.lod; }
size_t astc_decode_lod_grad_bytes(const DecodeLodGradLaunch* grids, uint32_t count);
uint32_t astc_decode_lod_grad_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                    const DecodeLodGradLaunch* grids, uint32_t count);
int astc_decode_lod_grad_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* Cube maps sampled by direction at a level of detail per point (astcenc_amd_sample_cube_tensors_device; decode_cube.h,
 * kernel_decode_cube.hip): the lod call's sampler, without address modes, and launch, checked by the entry point -- as the lod
 * call's, and: every level square, no larger than 65536, with layers 6 z .. 6 z + 5 (z: the cube); the directions aligned to a float,
 * their pitch at least 3 out_x.  Work items, table and launch as the lod call's. */
size_t astc_decode_cube_bytes(const DecodeLodLaunch* grids, uint32_t count);
uint32_t astc_decode_cube_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                const DecodeLodLaunch* grids, uint32_t count);
int astc_decode_cube_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* Volumes sampled at (u, v, w) at a level of detail per point (astcenc_amd_sample_volume_tensors_device; decode_volume.h,
 * kernel_decode_volume.hip): the lod call's sampler, with address_z, and launch, checked by the entry point -- as the lod call's
 * without a slice, and: any footprint, 2D or 3D; every level no larger than 65536 along x, y and z and of fewer than 2^32 - 1
 * blocks, layers of block_z slices counted; the triples aligned to a float, their pitch at least 3 out_x.  Work items, table and
 * launch as the lod call's. */
size_t astc_decode_volume_bytes(const DecodeLodLaunch* grids, uint32_t count);
uint32_t astc_decode_volume_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                  const DecodeLodLaunch* grids, uint32_t count);
int astc_decode_volume_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* The gradients of that call (astcenc_amd_sample_volume_grad_device; decode_volume_grad.h, kernel_decode_volume_grad.hip): the
 * volume call's sampler and the lod gradient's launch, its z unused, checked by the entry point: the volume call's checks with
 * grad_out in the place of the output -- it is read -- grad_coords aligned to a float and triples, its pitch at least 3 out_x,
 * grad_lod (when given) aligned to a float, the pitches resolved.  Work items, table and launch as the volume call's. */
size_t astc_decode_volume_grad_bytes(const DecodeLodGradLaunch* grids, uint32_t count);
uint32_t astc_decode_volume_grad_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                       const DecodeLodGradLaunch* grids, uint32_t count);
int astc_decode_volume_grad_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream);
/* The per-footprint tables of the decoder (block mode field -> weight grid, bit budget -> colour quant level): built on
 * the host once per context into astc_decode_tables_bytes() bytes, uploaded with the context's other tables. */
size_t astc_decode_tables_bytes();
void astc_decode_tables_build(void* out, uint32_t block_x, uint32_t block_y, uint32_t block_z);

/* Block quality launch (kernel_quality.hip): an image set's table as for the decoder (astc_quality_set_bytes(count) bytes),
 * one QualityLaunch per entry (decode.d_image and decode.stream unused).  astc_quality_set_launch queues the kernels from the
 * table's host and device copies (d_table: null for a set of one entry, whose record travels with the launch): d_partials = astc_quality_scratch_doubles() doubles, d_sums = METRIC_SUMS_HOST doubles per
 * entry, which receive the totals. */
struct QualityLaunch {
	DecodeLaunch decode;
	const void* d_original; uint32_t original_type;
	double* d_block_errors;
};
size_t astc_quality_set_bytes(uint32_t count);
size_t astc_quality_scratch_doubles();
uint32_t astc_quality_set_build(void* out, const QualityLaunch* entries, uint32_t count);
int astc_quality_set_launch(const void* h_table, const void* d_table, double* d_partials, double* d_sums, int hdr, int fstop_lo, int fstop_hi, void* stream);

/* Block selection (kernel_select.hip, block_select.h).  astc_select_launch queues the count, scan and scatter kernels:
 * d_list[0 .. n) receives the ascending indices of the selected blocks, d_counts (astc_select_scratch_words(blocks) words) ends in
 * n at word astc_select_total_word(blocks).  astc_merge_launch: for each of the *d_count listed blocks whose `strong` record is
 * strictly better than its `base` record, the 16 bytes of d_strong replace those of d_out and the record replaces the base
 * one (d_base_errors is updated in place); *d_replaced counts them (zeroed by the launch). */
struct SelectLaunch {
	const double* d_errors;
	uint32_t dim_x, dim_y, dim_z, block_x, block_y, block_z, blocks;
	double weight[4], max_mse;
	uint32_t* d_list;
	uint32_t* d_counts;
	void* stream;
};
size_t astc_select_scratch_words(size_t blocks);
size_t astc_select_total_word(size_t blocks);
int astc_select_launch(const SelectLaunch& s);
struct MergeLaunch {
	const uint32_t* d_list; const uint32_t* d_count;
	uint32_t blocks;                 // of the image: a list entry past them is skipped
	uint32_t max_count;              // the grid covers this many list positions (the host's copy of *d_count)
	const double* d_strong_errors; double* d_base_errors;
	const uint8_t* d_strong; uint8_t* d_out;
	double weight[4];
	uint32_t* d_replaced;
	void* stream;
};
int astc_merge_launch(const MergeLaunch& m);

/* Block selection over an image set with a block budget, and the merge over a set (kernel_select_set.hip, block_budget.h).
 * astc_budget_table_build writes the set's table (astc_budget_table_bytes(count) bytes: ImageSetTable, first[], one BudgetEntry per
 * entry) on the host.  astc_budget_select_launch queues the selection from the table's device copy: d_list[0 .. n) receives the
 * ascending global indices of the selected blocks; d_keys: 8 bytes per block; d_counts: astc_budget_count_words(blocks) words;
 * d_fixed: astc_budget_fixed_bytes() bytes (the state and the histograms), in which astc_budget_counts() points at two words,
 * the candidate count and n.  astc_merge_set_launch: astc_merge_launch over the set, d_strong and both record arrays indexed by
 * the global block, the bytes stored into the entries' own buffers (the table's `out`); the list's length is read from d_fixed. */
struct BudgetSetEntry {
	uint32_t dim_x, dim_y, dim_z;
	uint8_t* device_out;             // the merge only
};
struct BudgetSelectLaunch {
	const double* d_errors;
	const uint8_t* d_table;
	uint32_t block_x, block_y, block_z, blocks;
	double weight[4], max_mse;
	uint32_t max_blocks;             // 0xFFFFFFFF: no budget
	unsigned long long* d_keys;
	uint32_t* d_counts;
	uint8_t* d_fixed;
	uint32_t* d_list;
	void* stream;
};
size_t astc_budget_table_bytes(uint32_t count);
void astc_budget_table_build(void* out, const BudgetSetEntry* entries, uint32_t count, uint32_t block_x, uint32_t block_y, uint32_t block_z);
size_t astc_budget_count_words(size_t blocks);
size_t astc_budget_fixed_bytes();
const uint32_t* astc_budget_counts(const uint8_t* d_fixed);
int astc_budget_select_launch(const BudgetSelectLaunch& s);
struct MergeSetLaunch {
	const uint32_t* d_list;
	const uint8_t* d_fixed;
	uint32_t max_count;              // the grid covers this many list positions (the host's copy of the list's length)
	const double* d_strong_errors; double* d_base_errors;
	const uint8_t* d_strong;
	const uint8_t* d_table;
	double weight[4];
	uint32_t* d_replaced;
	void* stream;
};
int astc_merge_set_launch(const MergeSetLaunch& m);

/* Mip chain generation (kernel_mips.hip): queues the launches of `job` on `stream` (job.stream unused), level i made from level
 * i - 1.  d_srgb: the tables of astc_mip_srgb_tables_build in device memory (astc_mip_srgb_table_bytes()), used for RGBA8 when
 * job.srgb != 0. */
int astc_mip_launch(const MipChainJob& job, const void* d_srgb, void* stream);
size_t astc_mip_srgb_table_bytes();
void astc_mip_srgb_tables_build(void* out);
/* ... of the box filter with alpha-weighted colour (kernel_mip_weighted.hip, job.weight != 0 and job.filter_kind == 0). */
int astc_mip_weighted_launch(const MipChainJob& job, const void* d_srgb, void* stream);
/* ... with a windowed filter (kernel_mip_filter.hip, job.filter_kind != 0): astc_mip_filter_table_build writes the taps of every
 * level into `out` on the host (0; 1 when they would exceed the library's 64 MiB scratch bound, nothing built; 2 on an internal
 * limit), astc_mip_filter_launch queues the levels from the table's device copy d_table; astc_mip_filter_weighted_launch does
 * from the same table when job.weight != 0 (kernel_mip_weighted.hip). */
int astc_mip_filter_table_build(const MipChainJob& job, std::vector<uint8_t>& out);
int astc_mip_filter_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream);
int astc_mip_filter_weighted_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream);
/* ... with job.filter_edge == MIP_EDGE_CUBE (kernel_mip_cube.hip), plain or weighted, from the same table: an ARRAY of square
 * layers, six to a cube (the caller has checked it). */
int astc_mip_cube_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream);
/* ... and its post-passes (kernel_mip_post.hip), queued after the generation of the same job when job.post_flags != 0.
 * d_scratch: astc_mip_post_scratch_bytes(job) bytes of device memory (0 when no scratch is needed; never above 64 MiB). */
size_t astc_mip_post_scratch_bytes(const MipChainJob& job);
int astc_mip_post_launch(const MipChainJob& job, void* d_scratch, void* stream);

/* Resizing (kernel_resize.hip): astc_resize_table_build writes the taps of the job's axes into `out` on the host (0; 1 when
 * they would exceed the library's 64 MiB scratch bound, nothing built), astc_resize_launch queues the kernel from the table's
 * device copy d_table. */
int astc_resize_table_build(const ResizeJob& job, std::vector<uint8_t>& out);
int astc_resize_launch(const ResizeJob& job, const void* d_table, const void* d_srgb, void* stream);

/* Image comparison launch (kernel_metrics.hip); d_sums = astc_compare_scratch_doubles() doubles of device memory,
 * the totals arrive in the first ten. */
struct CompareLaunch {
	const void* d_a; uint32_t type_a;
	const void* d_b; uint32_t type_b;
	size_t texels;
	double* d_sums;
	void* stream;
	int hdr, fstop_lo, fstop_hi;
};
int astc_compare_launch(const CompareLaunch& c);
size_t astc_compare_scratch_doubles();

} // namespace astcd
